"""GPU: the temporal accumulation of the denoiser (vr_denoise_temporal / vr_denoise_history / vr_denoise_history_reset) through the C ABI: the first
call is vr_denoise; the kernel equals the host-compiled lane code bit for bit over moving sequences (tests/hostkernel/temporal_host.cpp, itself held to
a float64 statement by tests/test_temporal_host.py); a fixed camera is a running mean; what keeps and what drops the history; that it helps where it
should; the Python, volpy and CLI interfaces."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hk_adaptive
import hk_denoise
import hk_temporal as ht
import scenes
import volren_amd
from gpu_frames import _camera, _check_against_replay, _frame, _orbit, _scene
from hk_common import same as _same

pytestmark = pytest.mark.gpu


# ---- 4: the first call is vr_denoise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
@pytest.mark.parametrize("iterations", (0, 1, 5))
def test_first_call_equals_denoise(name, iterations):
    r = _scene(name, 64, 48)
    _frame(r, 8)
    r.denoise_iterations = iterations
    r.denoise()
    spatial = r.denoised()
    r.denoise_temporal()
    assert _same(r.denoised(), spatial), (name, iterations)
    c, v, n = r.denoise_history()
    assert _same(c, r.framebuffer())
    assert _same(v, hk_denoise.prepare(r.variance(), r.features(), r.sample)[0])
    assert (n == 1).all() and n.dtype == np.float32


# ---- 5: the kernel is the host lane code, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
def test_moving_sequence_matches_the_host_lane_code(name):
    r = _scene(name, 64, 48)
    replay = ht.Replay()
    longest = 0
    for i in range(4):
        _orbit(r, 2.0 * i)
        _frame(r, 6, seed=i + 1)
        r.denoise_temporal()
        n, _ = _check_against_replay(r, replay, (name, i))
        longest = max(longest, int(n.max()))
    assert longest >= 3, longest                     # histories were found and followed, not rejected everywhere


def test_sequence_with_a_change_of_fov_and_a_camera_that_looks_away():
    r = _scene("c1", 64, 48)
    replay = ht.Replay()
    for i, (fov, yaw) in enumerate(((40.0, 0.0), (55.0, 0.0), (30.0, 4.0), (40.0, 35.0), (40.0, 150.0), (40.0, 0.0))):
        r.cam_fov = fov
        _orbit(r, 1.5 * i, yaw)
        _frame(r, 4, seed=i + 1)
        prev = replay.hist
        r.denoise_temporal()
        n, _ = _check_against_replay(r, replay, (fov, yaw))
        if prev is not None:
            g = hk_denoise.prepare(r.variance(), r.features(), r.sample)[1]
            u, w, _, ok = ht.reproject(_camera(r), prev[0], g[..., 3], g[..., 7])
            off = ok & ((u < -1) | (u >= 64) | (w < -1) | (w >= 48))
            if yaw == 35.0:
                assert off.any() and (n[off] == 1).all()      # part of the frame saw something else before
            if yaw == 150.0:
                assert (~ok).any() and (n[~ok] == 1).all()    # behind the previous camera
            if i == 1:
                assert (n == 2).any()


@pytest.mark.parametrize("w,h", ((1, 1), (1, 37), (37, 1), (15, 9), (17, 16), (33, 31), (1030, 770)))
def test_small_thin_and_large_frames(w, h):
    r = _scene("c1", w, h)
    replay = ht.Replay()
    for i in range(2 if w * h > 100000 else 3):
        _orbit(r, 2.0 * i)
        _frame(r, 2 if w * h > 100000 else 5, seed=i + 1)
        r.denoise_temporal()
        _check_against_replay(r, replay, (w, h, i))


def test_a_ragged_frame_as_the_second_frame():
    W, H = 64, 48
    r = _scene("c4_64", W, H)
    replay = ht.Replay()
    _frame(r, 8, seed=1)
    r.denoise_temporal()
    _check_against_replay(r, replay, "uniform")
    _orbit(r, 2.0)
    r.seed = 2
    r.reset()
    r.render_adaptive(2, 8, 0.0)
    r.set_tiles([1, 2, 7])
    r.render_adaptive(2, 32, 0.0)
    r.set_tiles([])
    counts = r.tile_samples()
    assert sorted(set(counts.reshape(-1).tolist())) == [8, 32]
    r.render_features(8)
    r.denoise_temporal()
    n, _ = _check_against_replay(r, replay, "ragged", n=hk_adaptive.per_pixel(counts, W, H))
    assert (n == 2).any()


# ---- 6: a fixed camera is a running mean --------------------------------------------------------------------------------------------------------------
def test_a_fixed_camera_is_a_running_mean():
    """alpha = 2^-20, so a = 1 / N: after K frames C is the mean of the K framebuffers and V = sum v_i / K^2, up to rounding.  Roundings of one blend
    (vr_temporal.h step 4), each at most 2^-24 of the largest value M the channel takes in any frame (every operand is a convex combination of such):
      C: a = 1 / N, 1 - a, the two products, the sum                                                   -> 5 x 2^-24 M
      V: a and 1 - a each enter squared (2 each), the two squares, the two products, the sum             -> 9 x 2^-24 M
    An error made in one blend is scaled by 1 - a <= 1 in the next, so K - 1 blends give (K - 1) times that (first order; the second order is 2^-48)."""
    K, W, H = 6, 64, 48
    r = _scene("c2", W, H)
    r.denoise_alpha = 2.0 ** -20
    fbs, vs = [], []
    for i in range(K):
        _frame(r, 8, seed=i + 1, fseed=99)           # the same features every frame: every depth and coverage test passes by construction
        r.denoise_temporal()
        fbs.append(r.framebuffer().astype(np.float64))
        vs.append(hk_denoise.prepare(r.variance(), r.features(), r.sample)[0].astype(np.float64))
    c, v, n = r.denoise_history()
    assert (n == K).all()
    eps = 2.0 ** -24 * (1.0 + 2.0 ** -20)
    for ch in range(4):
        M = max(f[..., ch].max() for f in fbs)
        err = np.abs(c[..., ch] - np.mean([f[..., ch] for f in fbs], axis=0)).max()
        print("channel %d: largest error %.3g, bound %.3g" % (ch, err, (K - 1) * 5 * eps * M))
        assert err <= (K - 1) * 5 * eps * M, (ch, err, M)
    Mv = max(x.max() for x in vs)
    err = np.abs(v - np.sum(vs, axis=0) / K ** 2).max()
    print("variance: largest error %.3g, bound %.3g" % (err, (K - 1) * 9 * eps * Mv))
    assert err <= (K - 1) * 9 * eps * Mv, (err, Mv)
    assert not _same(fbs[0], fbs[1])
    r.denoise_alpha = 1.0                            # 0 * h + 1 * c with h finite: the current frame, bit for bit
    _frame(r, 8, seed=K + 1, fseed=99)
    r.denoise_temporal()
    c, v, n = r.denoise_history()
    assert _same(c, r.framebuffer()) and (n == K + 1).all()
    assert _same(v, hk_denoise.prepare(r.variance(), r.features(), r.sample)[0])


# ---- 7: state rules -------------------------------------------------------------------------------------------------------------------------------------
def test_what_keeps_and_what_drops_the_history():
    r = _scene("c1", 48, 40)
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    _frame(r, 4, seed=1, fseed=7)
    r.denoise_temporal()
    want = 1
    assert (r.denoise_history()[2] == want).all()
    for change in ("reset", "cam_pos", "envmap", "commit"):
        if change == "reset":
            r.reset()
        elif change == "cam_pos":
            r.cam_pos = r.cam_pos                    # set, to the same value: the camera stays byte-equal
        elif change == "envmap":
            r.load_envmap(scenes.HDR)
        else:
            r.commit()
        _frame(r, 4, seed=want + 1, fseed=7)
        r.denoise_temporal()
        want += 1
        assert (r.denoise_history()[2] == want).all(), change
    # vr_denoise in between neither reads nor writes it
    before = r.denoise_history()
    r.denoise()
    spatial = r.denoised()
    assert all(_same(a, b) for a, b in zip(before, r.denoise_history()))
    assert _same(spatial, hk_denoise.denoise(r.framebuffer(), r.variance(), r.features(), r.sample, r.denoise_iterations, tuple(r.denoise_sigma)))
    # a moved camera keeps it too: what no longer matches is for the taps to reject
    _orbit(r, 1.0)
    _frame(r, 4, seed=9, fseed=7)
    r.denoise_temporal()
    assert r.denoise_history()[2].max() == want + 1
    # dropped by the reset call and by resize
    r.denoise_history_reset()
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    r.denoised()                                     # the last result is still there
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 1).all()
    r.denoise_temporal()                             # twice on one frame: the frame blended with itself
    assert (r.denoise_history()[2] == 2).all()
    r.resize(40, 32)
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    _frame(r, 4)
    r.denoise_temporal()
    c, v, n = r.denoise_history()
    assert c.shape == (32, 40, 4) and (n == 1).all()


def test_denoise_temporal_leaves_the_frame_alone():
    r = _scene("c3", 48, 40)
    _frame(r, 8)
    r.draw()
    fb, var, feat, disp = r.framebuffer(), r.variance(), r.features(), r.display()
    for _ in range(2):
        r.denoise_temporal()
        assert _same(r.framebuffer(), fb) and _same(r.variance(), var) and _same(r.features(), feat) and _same(r.display(), disp)
    r.draw()
    assert _same(r.display(), disp)


def test_refusals_and_recovery():
    """the refusals of test_gpu_denoise.py::test_refusals_and_recovery, for the new call, with its own name in the message"""
    r = scenes.hip_scene("c1", 32, 32)
    r.variance = 1
    r.render(4)
    with pytest.raises(volren_amd.VolrenError, match="denoise_temporal: no feature pass"):
        r.denoise_temporal()
    r.render_features(4)
    r.denoise_temporal()
    r.denoised()
    r.resize(48, 32)                                         # drops the features, the denoised buffer and the history
    with pytest.raises(volren_amd.VolrenError, match="denoise"):
        r.denoised()
    r.render(4)
    with pytest.raises(volren_amd.VolrenError, match="denoise_temporal: no feature pass"):
        r.denoise_temporal()
    r.render_features(4)
    r.reset()
    with pytest.raises(volren_amd.VolrenError, match="denoise_temporal: .*sample < 1"):
        r.denoise_temporal()
    r.variance = 0
    r.render(2)
    r.variance = 1
    r.render(2)                                              # moments switched on mid-frame
    with pytest.raises(volren_amd.VolrenError, match="denoise_temporal.*moments"):
        r.denoise_temporal()
    r.reset()
    r.render(4)
    r.set_tiles([0, 2])
    with pytest.raises(volren_amd.VolrenError, match="denoise_temporal: a tile subset"):
        r.denoise_temporal()
    r.set_tiles([])
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()                                  # none of the refused calls made one
    r.reset()
    r.render(4)
    r.denoise_temporal()
    assert _same(r.denoised(), hk_denoise.denoise(r.framebuffer(), r.variance(), r.features(), r.sample, r.denoise_iterations, tuple(r.denoise_sigma)))


def test_denoise_alpha_range_checks():
    lib = volren_amd.load()
    r = volren_amd.Renderer(16, 16)
    assert r.denoise_alpha == np.float32(0.1)
    for v in (2.0 ** -20, 0.05, 1.0):
        r.denoise_alpha = v
        assert r.denoise_alpha == np.float32(v)
    r.denoise_alpha = 0.25
    for bad in (0.0, -0.5, np.nextafter(np.float32(2.0 ** -20), np.float32(0)), np.nextafter(np.float32(1), np.float32(2)), np.inf, np.nan):
        v = np.asarray([bad], np.float32)
        assert lib.vr_set_float(r._h, b"denoise_alpha", v.ctypes.data_as(C.POINTER(C.c_float)), 1) == 1, bad
        assert b"denoise_alpha" in lib.vr_last_error() and b"2^-20" in lib.vr_last_error()
        assert r.denoise_alpha == 0.25
    v = np.asarray([0.5, 0.5], np.float32)
    assert lib.vr_set_float(r._h, b"denoise_alpha", v.ctypes.data_as(C.POINTER(C.c_float)), 2) == 1
    assert r.denoise_alpha == 0.25


def test_a_history_that_does_not_fit_fails_the_call_and_changes_nothing():
    lib = volren_amd.load()
    r = _scene("c1", 64, 48)
    _frame(r, 4, seed=1, fseed=7)                    # the same features in both frames: every tap counts
    r.denoise_temporal()
    before, result = r.denoise_history(), r.denoised()
    _frame(r, 4, seed=2, fseed=7)
    try:
        lib.vr_test_alloc_cap_mb(0)                  # the second half of the history pair cannot be allocated
        with pytest.raises(volren_amd.VolrenError, match="allocation cap"):
            r.denoise_temporal()
    finally:
        lib.vr_test_alloc_cap_mb(-1)
    assert all(_same(a, b) for a, b in zip(before, r.denoise_history()))
    assert _same(result, r.denoised())
    r.denoise_temporal()                             # and with the memory back, the sequence goes on
    assert (r.denoise_history()[2] == 2).all()
    fresh = _scene("c1", 64, 48)
    _frame(fresh, 4)
    try:
        lib.vr_test_alloc_cap_mb(0)
        with pytest.raises(volren_amd.VolrenError, match="allocation cap"):
            fresh.denoise_temporal()                 # the first call: no history comes of it
    finally:
        lib.vr_test_alloc_cap_mb(-1)
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        fresh.denoise_history()


# ---- 8: it helps, where it should -----------------------------------------------------------------------------------------------------------------------
def _quality(step_degrees, frames=6, size=256, spp=16):
    """-> (raw, spatial, temporal) relative L2 of the last of `frames` frames against 1024 spp of seed 777 at the last camera, and the last history length"""
    r = _scene("c2", size, size)
    for i in range(frames):
        _orbit(r, step_degrees * i)
        _frame(r, spp, seed=i + 1)
        r.denoise_temporal()
    temporal, (_, _, n) = r.denoised(), r.denoise_history()
    r.denoise()
    spatial, raw, k = r.denoised(), r.framebuffer(), r.features()[..., 3]
    ref = scenes.hip_scene("c2", size, size)
    _orbit(ref, step_degrees * (frames - 1))
    ref.seed = 777
    ref.render(1024)
    want = ref.framebuffer()[..., :3]
    return tuple(scenes.rel_l2(x[..., :3], want) for x in (raw, spatial, temporal)), n, k


def test_a_fixed_camera_beats_the_spatial_filter():
    """c2 at 256^2, 6 frames of 16 spp (features 16 spp), fixed camera, against 1024 spp of seed 777; the yardstick is denoise() of the same last frame.
    Measured on an MI355X: raw 0.1203, spatial 0.0397, temporal 0.0284, ratio temporal / spatial 0.716 (a CPU prototype gave 0.74); the bound is
    halfway between that and 1."""
    (raw, spatial, temporal), n, _ = _quality(0.0)
    print("fixed camera: raw %.4f spatial %.4f temporal %.4f ratio %.3f, mean N %.2f" % (raw, spatial, temporal, temporal / spatial, n.mean()))
    assert temporal <= 0.858 * spatial, (raw, spatial, temporal)


def test_a_slow_orbit_beats_the_spatial_filter_and_keeps_its_history():
    """The same with the camera turned 1 degree about +y per frame (cam_pos = (1, 0, 1) turned, cam_dir towards the origin).
    Measured on an MI355X: raw 0.1181, spatial 0.0398, temporal 0.0332, ratio 0.834 (a CPU prototype gave 0.87); the bound is halfway between that
    and 1.  At 2 degrees per frame and this size the history lags too far and the call loses to the spatial filter: DESIGN.md 5 has the table.
    It must not pass by rejecting everything: at least half of the pixels that show the volume have three or more frames behind them (measured: 97.5 %,
    mean N 5.25 of 6, 4.0 % of all pixels without history)."""
    (raw, spatial, temporal), n, k = _quality(1.0)
    hit = k > 0
    print("1 degree per frame: raw %.4f spatial %.4f temporal %.4f ratio %.3f; N >= 3 on %.1f %% of the volume's pixels, mean N %.2f, %.1f %% of all pixels without history"
          % (raw, spatial, temporal, temporal / spatial, 100.0 * (n[hit] >= 3).mean(), n.mean(), 100.0 * (n == 1).mean()))
    assert hit.any() and (n[hit] >= 3).mean() >= 0.5
    assert temporal <= 0.917 * spatial, (raw, spatial, temporal)


# ---- 9: Python, volpy, CLI --------------------------------------------------------------------------------------------------------------------------------
def test_python_and_volpy_shapes_and_row_order():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.variance = 1
    for _ in range(2):
        vr.render(6)
        vr.render_features(6)
        vr.denoise_temporal()
    r = vr._r
    c, v, n = r.denoise_history()
    assert c.shape == (24, 40, 4) and v.shape == (24, 40) and n.shape == (24, 40) and c.dtype == v.dtype == n.dtype == np.float32
    raw_c, raw_v, raw_n = np.empty(24 * 40 * 4, np.float32), np.empty(24 * 40, np.float32), np.empty(24 * 40, np.float32)
    assert r._L.vr_denoise_history(r._h, raw_c.ctypes.data, raw_v.ctypes.data, raw_n.ctypes.data) == 0
    assert np.array_equal(c.reshape(-1), raw_c) and np.array_equal(v.reshape(-1), raw_v) and np.array_equal(n.reshape(-1), raw_n)
    only_n = np.empty(24 * 40, np.float32)
    assert r._L.vr_denoise_history(r._h, None, None, only_n.ctypes.data) == 0 and np.array_equal(only_n, raw_n)      # any pointer may be NULL
    assert (n == 2).all()
    # row 0 = bottom, like framebuffer(): with alpha = 1 the history is the frame
    r.denoise_alpha = 1.0
    vr.render(6)
    vr.render_features(6)
    vr.denoise_temporal()
    assert np.array_equal(r.denoise_history()[0], r.framebuffer())
    dd = vr.denoised_data()
    assert dd.shape == (40, 24, 3) == vr.fbo_data().shape
    assert np.array_equal(dd.reshape(-1), r.denoised()[..., :3].reshape(-1))
    vr.denoise_history_reset()
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()


def test_cli_denoise_temporal(tmp_path):
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "12", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]

    def run(inputs, flag, png, extra=()):
        out = subprocess.run([exe] + inputs + list(extra) + args + [flag, "--output", png + ".png"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        return out

    for flag, png in (("--denoise", "dn"), ("--denoise-temporal", "dt")):
        out = run([scenes.SMOKE, scenes.HDR], flag, png)
        assert out.returncode == 0, out.stderr[-2000:]
    assert (tmp_path / "dn_000000.png").read_bytes() == (tmp_path / "dt_000000.png").read_bytes()      # one frame: the same picture
    # a folder of two grid frames: the first frame as --denoise, the second blended with the first
    lib = volren_amd.load()
    folder = tmp_path / "anim"
    folder.mkdir()
    for i, s in enumerate((5, 6)):
        f = scenes.synthetic_density(40, seed=s)
        assert lib.vr_write_brick_from_dense(f.ctypes.data, 40, 40, 40, None, str(folder / ("f%03d.brick" % i)).encode()) == 0
    for flag, png in (("--denoise", "an"), ("--denoise-temporal", "at")):
        out = run([str(folder), scenes.HDR], flag, png)
        assert out.returncode == 0, out.stderr[-2000:]
    assert (tmp_path / "an_000000.png").read_bytes() == (tmp_path / "at_000000.png").read_bytes()
    assert (tmp_path / "an_000001.png").read_bytes() != (tmp_path / "at_000001.png").read_bytes()
    bad = run([scenes.SMOKE, scenes.HDR], "--denoise-temporal", "bad", extra=("--gpus", "2"))
    assert bad.returncode != 0 and "--denoise-temporal renders on one device only" in bad.stderr
