"""GPU: adaptive sampling per 16x16 tile (vr_render_adaptive, vr_tile_samples, vr_tile_error) against a host replay of its schedule fed with the
error estimate of the host-compiled lane code (tests/hostkernel/adaptive_host.cpp) on uniform frames; a tile at n samples is bit for bit the tile
of an n-spp frame, moments included.  Ragged frames: refusals, variance, denoiser.  The Python, volpy and CLI interfaces."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hk_adaptive as ha
from hk_common import bits as _bits
import scenes
import volren_amd

pytestmark = pytest.mark.gpu

W, H = 72, 56                                              # 5 x 4 tiles, the last column 8 wide, the top row 8 high
COUNTS = (4, 8, 16, 32, 64)


def _uniform(name):
    """uniform frames at 4 .. 64 spp with variance: {n: (framebuffer, variance, e_t of the host build, vr_tile_error)}"""
    r = scenes.hip_scene(name, W, H)
    r.variance = 1
    out, have = {}, 0
    for n in COUNTS:
        r.render(n - have)
        have = n
        fb, var = r.framebuffer(), r.variance()
        out[n] = (fb, var, ha.tile_error(fb, var, n, from_variance=True), r.tile_error())
        assert np.array_equal(r.tile_samples(), np.full(ha.tiles_of(W, H), n, np.int32))
    return r, out


def _err_at(frames):
    tx = ha.tiles_of(W, H)[1]
    return lambda t, n: float(frames[n][2][t // tx, t % tx])


def _pick_threshold(frames, start, set_ids, min_spp, want_groups=False):
    """a threshold from the data for which the replay spreads the counts (want_groups: has a round with several count groups instead)"""
    vals = np.concatenate([frames[n][2][np.isfinite(frames[n][2])].ravel() for n in (8, 16, 32)])
    for q in np.linspace(0.05, 0.95, 19):
        t = float(np.float32(np.quantile(vals, q)))
        n, rounds, hist = ha.replay(_err_at(frames), start, set_ids, min_spp, 64, t)
        spread = len(set(int(n[i]) for i in set_ids)) >= 2
        if (any(len(g) >= 2 for g in hist) if want_groups else spread):
            return t, n, rounds
    raise AssertionError("no threshold spreads the counts")


def _same_tiles(frame, frames, counts, which):
    tx = ha.tiles_of(W, H)[1]
    for t, n in enumerate(counts.reshape(-1)):
        y, x = (t // tx) * 16, (t % tx) * 16
        want = frames[int(n)][which]
        assert np.array_equal(_bits(frame[y:y + 16, x:x + 16]), _bits(want[y:y + 16, x:x + 16])), (t, int(n), which)


@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
def test_schedule_equals_the_host_replay_bit_for_bit(name):
    r, frames = _uniform(name)
    for n in COUNTS:                                       # vr_tile_error on uniform frames = the host build
        assert np.array_equal(_bits(frames[n][3]), _bits(frames[n][2])), n
    n_all = int(np.prod(ha.tiles_of(W, H)))
    every = list(range(n_all))
    t, want, rounds = _pick_threshold(frames, [0] * n_all, every, 4)
    r.reset()
    r.variance = 0                                         # render_adaptive keeps the moments whatever the setting says
    r.render_adaptive(4, 64, t)
    got = r.tile_samples()
    assert np.array_equal(got.reshape(-1), want), (name, t)
    assert len(set(got.reshape(-1).tolist())) >= 2
    assert r.sample == int(want.max()) and r.adaptive_rounds == rounds and r.get_int("variance") == 0
    _same_tiles(r.framebuffer(), frames, got, 0)
    _same_tiles(r.variance(), frames, got, 1)
    assert r.last_kernel_ms() > 0 and 0 < r.last_pathtrace_ms() <= r.last_kernel_ms()
    # continuation: uniform 8 spp, then adaptive from min_spp 8 = adaptive from scratch with min_spp 8
    r.reset()
    r.render_adaptive(8, 64, t)
    scratch_n, scratch_fb, scratch_var = r.tile_samples(), r.framebuffer(), r.variance()
    r.reset()
    r.variance = 1
    r.render(8)
    r.render_adaptive(8, 64, t)
    assert np.array_equal(r.tile_samples(), scratch_n)
    assert np.array_equal(_bits(r.framebuffer()), _bits(scratch_fb)) and np.array_equal(_bits(r.variance()), _bits(scratch_var))
    # a call on a ragged frame of tiles at 8, 16 and 32 samples: several count groups in one round
    r.reset()
    r.render(8)
    r.set_tiles([0, 5, 10, 15])
    r.render_adaptive(8, 16, 0.0)
    r.set_tiles([1, 6, 11, 16])
    r.render_adaptive(8, 32, 0.0)
    r.set_tiles([])
    start = r.tile_samples().reshape(-1)
    assert sorted(set(start.tolist())) == [8, 16, 32]
    _same_tiles(r.framebuffer(), frames, start, 0)
    t2, want2, _ = _pick_threshold(frames, start, every, 8, want_groups=True)
    r.render_adaptive(8, 64, t2)
    got2 = r.tile_samples()
    assert np.array_equal(got2.reshape(-1), want2), (name, t2)
    _same_tiles(r.framebuffer(), frames, got2, 0)
    _same_tiles(r.variance(), frames, got2, 1)


def test_threshold_zero_is_a_uniform_frame_and_render_may_follow():
    r = scenes.hip_scene("c1", W, H)
    r.render_adaptive(4, 64, 0.0)
    assert r.sample == 64 and (r.tile_samples() == 64).all() and r.adaptive_rounds == 4
    ref = scenes.hip_scene("c1", W, H)
    ref.variance = 1
    ref.render(64)
    assert np.array_equal(_bits(r.framebuffer()), _bits(ref.framebuffer()))
    assert np.array_equal(_bits(r.variance()), _bits(ref.variance()))
    r.variance = 1
    r.render(8)                                            # a uniform frame: render goes on
    ref.reset()
    ref.render(72)
    assert r.sample == 72 and np.array_equal(_bits(r.framebuffer()), _bits(ref.framebuffer()))
    assert np.array_equal(_bits(r.variance()), _bits(ref.variance()))


def test_tile_subset_leaves_the_other_tiles_alone():
    r, frames = _uniform("c3")
    n_all = int(np.prod(ha.tiles_of(W, H)))
    subset = [0, 3, 6, 7, 12, 18, 19]
    t, want, _ = _pick_threshold(frames, [8] * n_all, subset, 8)
    r.reset()
    r.render(8)
    r.set_tiles(subset)
    r.render_adaptive(8, 64, t)
    got = r.tile_samples().reshape(-1)
    assert np.array_equal(got, want)
    assert all(got[i] == 8 for i in range(n_all) if i not in subset)
    _same_tiles(r.framebuffer(), frames, got, 0)
    _same_tiles(r.variance(), frames, got, 1)
    r.set_tiles([])


def test_refusals_and_recovery():
    r = scenes.hip_scene("c1", W, H)
    L, h = r._L, r._h
    for mn, mx, t in ((1, 64, 0.1), (9, 8, 0.1), (4, 64, -1e-3), (4, 64, float("nan")), (4, 64, float("inf"))):
        assert L.vr_render_adaptive(h, mn, mx, t) == 3, (mn, mx, t)          # VR_ERR_ARG
    buf = np.zeros(64, np.int32)
    assert L.vr_tile_samples(h, buf.ctypes.data, 19) == 3
    assert L.vr_tile_error(h, buf.ctypes.data, 21) == 3
    r.render(4)                                            # variance off: no moments
    with pytest.raises(volren_amd.VolrenError, match="moments"):
        r.render_adaptive(4, 64, 0.1)
    with pytest.raises(volren_amd.VolrenError, match="moments"):
        r.tile_error()
    r.reset()
    r.set_tiles([0, 1])                                    # a ragged frame: two tiles at 16, the rest at 0
    r.render_adaptive(16, 16, 0.1)
    r.set_tiles([])
    assert r.sample == 16 and r.tile_samples().reshape(-1).tolist() == [16, 16] + [0] * 18
    fb = r.framebuffer()
    with pytest.raises(volren_amd.VolrenError, match="render_adaptive"):
        r.render(4)
    with pytest.raises(volren_amd.VolrenError, match="render_adaptive"):
        r.trace()
    with pytest.raises(volren_amd.VolrenError, match="no samples"):
        r.render_features(4)
        r.denoise()
    assert r.sample == 16 and np.array_equal(_bits(r.framebuffer()), _bits(fb))
    assert np.isposinf(r.tile_error().reshape(-1)[2:]).all()
    r.sample = 16                                          # set by hand, even to the same value: a uniform frame again
    assert (r.tile_samples() == 16).all()
    r.reset()
    r.render(4)                                            # after reset: as today
    ref = scenes.hip_scene("c1", W, H)
    ref.render(4)
    assert np.array_equal(_bits(r.framebuffer()), _bits(ref.framebuffer()))


def test_denoise_on_a_ragged_frame_equals_the_host_lane_code():
    r = scenes.hip_scene("c4_64", W, H)
    r.render_adaptive(2, 32, 0.0)                          # uniform 32: then a subset goes further
    r.set_tiles([1, 2, 7, 11])
    r.render_adaptive(2, 128, 0.0)
    r.set_tiles([])
    counts = r.tile_samples()
    assert sorted(set(counts.reshape(-1).tolist())) == [32, 128]
    r.render_features(8)
    r.denoise()
    var = r.variance()
    n_px = ha.per_pixel(counts, W, H)
    assert (var[..., :3] > 0).any()
    want = ha.denoise(r.framebuffer(), var, r.features(), n_px, r.denoise_iterations, tuple(r.denoise_sigma))
    assert np.array_equal(_bits(r.denoised()), _bits(want))


def test_python_volpy_and_cli_interfaces(tmp_path):
    import volren_amd.volpy as volpy
    r = scenes.hip_scene("c1", 40, 24)
    r.render_adaptive(4, 16, 0.5)
    assert r.tile_samples().shape == (2, 3) and r.tile_samples().dtype == np.int32
    assert r.tile_error().shape == (2, 3) and r.tile_error().dtype == np.float32
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.render_adaptive(4, 4, 0.0)                          # a uniform frame of 4, then the top row's middle tile to 16
    vr._r.set_tiles([4])
    vr._r.render_adaptive(4, 16, 0.0)
    vr._r.set_tiles([])
    per_px = vr.sample_count_data()
    assert per_px.shape == (40, 24) == vr.fbo_data().shape[:2]
    grid = per_px.reshape(24, 40)                          # the same memory as fbo_data(): [H][W], row 0 = bottom
    assert (grid[16:24, 16:32] == 16).all() and grid.sum() == 16 * 8 * 16 + 4 * (24 * 40 - 8 * 16)
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "64", "-h", "48", "--render", "--spp", "32", "--bounces", "128", "--albedo", "0.8", "--density", "100", "--cam_fov", "40"]
    for extra, png in (([], "ad"), (["--denoise"], "dn")):
        out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--adaptive", "0.2", "--output", png + ".png"] + extra, cwd=tmp_path,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "spp mean" in out.stdout and (tmp_path / (png + "_000000.png")).exists()
    assert (tmp_path / "ad_000000.png").read_bytes() != (tmp_path / "dn_000000.png").read_bytes()
    bad = subprocess.run([exe, scenes.SMOKE, scenes.HDR, "--gpus", "2"] + args + ["--adaptive", "0.2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--adaptive" in bad.stderr
