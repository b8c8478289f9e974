"""GPU: the control variate on the expected coverage (vr_resolve / vr_resolved / vr_resolve_background, vr_filters.hip resolve_prepare_kernel and
resolve_kernel) bit for bit against the host build of the same header (tests/hostkernel/resolve_host.cpp, itself held to a float64 statement by
tests/test_resolve_host.py), on frames with partial tiles; "denoise_resolve" in front of vr_denoise and vr_denoise_temporal against the host filter run on
the host's resolved frame; every refusal on a live renderer; the sharded renderer; the Python, volpy and command-line layers."""
import subprocess

import numpy as np
import pytest

import hk_denoise
import hk_resolve as hr
import hk_temporal as ht
import scenes
import volren_amd
from gpu_frames import _camera
from hk_common import same as _same
from test_resolve_capi import check_setting

pytestmark = pytest.mark.gpu

W, H, SPP, RAYS = 72, 56, 4, 2                  # 5 x 4 tiles, the last column and the top row partial
SCENES = ("c2", "c3env", "c3", "c4_64")          # smoke.brick in front of the sky; under the LUT with the sky shown; under the LUT as configured (sky hidden); dense fp16


def _configure(x, name, is_oracle):
    scenes.configure(x, "c3" if name == "c3env" else name, is_oracle)
    if name == "c3env":
        x.show_environment = True if is_oracle else 1
    return x


def _pair(name, w=W, h=H):
    from oracle import binding as ob
    return _configure(volren_amd.Renderer(w, h), name, False), _configure(ob.OracleRenderer(w, h), name, True)


def _frame(r, spp=SPP, rays=RAYS, seed=None):
    if seed is not None:
        r.seed = seed
    r.reset()
    r.render(spp)
    r.render_features_expected(rays)


@pytest.mark.parametrize("name", SCENES)
def test_the_kernels_match_the_host_build_bit_for_bit(name):
    """B and y of a 72x56 frame of 4 spp against 2 x 2 expected rays; the framebuffer and the features are left as they were"""
    r, o = _pair(name)
    _frame(r)
    fb, guide = r.framebuffer(), r.features()
    want, want_b = hr.resolved(o, RAYS, fb, guide)
    r.resolve()
    assert _same(r.resolve_background(), want_b) and _same(r.resolved(), want)
    assert _same(r.framebuffer(), fb) and _same(r.features(), guide)
    assert _same(want[..., 3], guide[..., 3]) and not _same(want[..., :3], fb[..., :3])
    partial = (fb[..., 3] > 0) & (fb[..., 3] < 1)
    assert partial.sum() > 20                                        # the coin toss the call removes is in the frame
    if name == "c3":
        assert not want_b.any()                                      # the sky is hidden: B = 0
    else:
        assert (want_b[..., :3] > 0).all() and not want_b[..., 3].any()
    r.close()


# thin both ways, one pixel past a tile, one short of two tiles: the staged window's halo of 3 leaves the frame on each side in turn and crosses
# a tile edge with a partial tile next to it
@pytest.mark.parametrize("w,h", ((1, 37), (37, 1), (17, 16), (33, 31)))
def test_thin_and_one_past_a_tile_frames_match_the_host_build_bit_for_bit(w, h):
    r, o = _pair("c2", w, h)
    _frame(r, spp=2)
    fb, guide = r.framebuffer(), r.features()
    want, want_b = hr.resolved(o, RAYS, fb, guide)
    r.resolve()
    assert _same(r.resolve_background(), want_b) and _same(r.resolved(), want)
    r.close()


@pytest.mark.parametrize("name", SCENES)
def test_the_filter_starts_from_the_resolved_frame(name):
    """vr_denoise, then three frames of vr_denoise_temporal, with "denoise_resolve" 1: the host filter (hk_denoise, hk_temporal) run on the host's
    resolved frame with the frame's own variance, bit for bit; back at 0 vr_denoise gives the parent's frame again"""
    r, o = _pair(name)
    r.variance = 1
    _frame(r)
    r.denoise()
    parent = r.denoised()
    assert _same(parent, hk_denoise.denoise(r.framebuffer(), r.variance(), r.features(), r.sample, r.denoise_iterations, tuple(r.denoise_sigma)))
    r.denoise_resolve = 1
    r.denoise()
    y, _ = hr.resolved(o, RAYS, r.framebuffer(), r.features())
    assert _same(r.resolved(), y)
    assert _same(r.denoised(), hk_denoise.denoise(y, r.variance(), r.features(), r.sample, r.denoise_iterations, tuple(r.denoise_sigma)))
    assert not _same(r.denoised(), parent)
    replay = ht.Replay()
    for i in range(3):
        _frame(r, seed=100 + i)
        r.denoise_temporal()
        y, _ = hr.resolved(o, RAYS, r.framebuffer(), r.features())
        want = replay.frame(_camera(r), y, r.variance(), r.features(), r.sample, r.denoise_alpha, r.denoise_iterations, tuple(r.denoise_sigma))
        hc, hv, hn = r.denoise_history()
        for got, ref, part in ((hc, want[0], "C"), (hv, want[1], "V"), (hn, want[2], "N"), (r.denoised(), want[3], "denoised")):
            assert _same(got, ref), (name, i, part)
        assert (hn == i + 1).all()
    r.denoise_resolve = 0
    with pytest.raises(volren_amd.VolrenError, match="no history"):      # the change dropped it
        r.denoise_history()
    r.seed = 42
    _frame(r)
    r.denoise()
    assert _same(r.denoised(), parent)
    r.close()


def test_rejection_and_moments_start_from_it_too():
    """with "denoise_reject" 3 and with "denoise_moments" 1 the first frame's history colour is the resolved frame, and further frames run"""
    r, _ = _pair("c3env")
    r.variance = 1
    r.denoise_resolve = 1
    for setting, value in (("denoise_reject", 3.0), ("denoise_moments", 1)):
        setattr(r, setting, value)
        r.denoise_history_reset()
        for i in range(2):
            _frame(r, seed=7 + i)
            r.denoise_temporal()
            if i == 0:
                assert _same(r.denoise_history()[0], r.resolved()) and not _same(r.resolved(), r.framebuffer())
        assert (r.denoise_history()[2] == 2).mean() > 0.9 and np.isfinite(r.denoised()).all()      # (the rejection restarts a few pixels)
        setattr(r, setting, 0)
    r.close()


def test_every_refusal_on_a_live_renderer():
    """stochastic features last, one ray, a tile subset, integrator 2, no sample, after a resize -- each VR_ERR with its reason, through vr_resolve and
    through vr_denoise / vr_denoise_temporal with the setting on, and nothing launched: the last result stays"""
    r, _ = _pair("c3env", 48, 40)
    check_setting(r)
    r.variance = 1
    with pytest.raises(volren_amd.VolrenError, match="no resolve since the last resize"):
        r.resolved()
    with pytest.raises(volren_amd.VolrenError, match="no resolve since the last resize"):
        r.resolve_background()
    r.render_features_expected(2)
    with pytest.raises(volren_amd.VolrenError, match="holds no samples"):
        r.resolve()
    _frame(r)
    r.resolve()
    good = r.resolved()

    def refused(words):
        for call in (r.resolve, r.denoise, r.denoise_temporal):
            with pytest.raises(volren_amd.VolrenError, match=words):
                call()
        assert _same(r.resolved(), good)

    r.denoise_resolve = 1
    r.render_features(4)
    refused("not last filled by render_features_expected")
    r.render_features_expected(1)
    refused("rays >= 2 is needed")
    r.render_features_expected(2)
    r.set_tiles([0, 1])
    refused("tile subset")
    r.set_tiles([])
    r.integrator = 2
    refused("integrator = 2")
    r.integrator = 0
    r.resolve()
    r.denoise()
    r.resize(40, 24)
    r.reset()
    r.render(2)
    with pytest.raises(volren_amd.VolrenError, match="not last filled by render_features_expected"):
        r.resolve()
    with pytest.raises(volren_amd.VolrenError, match="no resolve since the last resize"):
        r.resolved()
    r.render_features_expected(2)
    r.resolve()
    assert r.resolved().shape == (24, 40, 4)
    r.close()


def test_a_ragged_frame_and_a_frame_of_one_pixel():
    r, o = _pair("c2", 48, 40)
    r.render_adaptive(2, 16, 0.05)
    assert len(set(r.tile_samples().reshape(-1).tolist())) > 1
    r.render_features_expected(2)
    r.resolve()
    assert _same(r.resolved(), hr.resolved(o, 2, r.framebuffer(), r.features())[0])
    for x in (r, o):
        x.resize(1, 1)
    _frame(r)
    r.resolve()
    assert _same(r.resolved(), hr.resolved(o, 2, r.framebuffer(), r.features())[0])
    r.close()


def test_two_logical_shards_equal_one_device():
    name, w, h = "c3env", 96, 64
    one, _ = _pair(name, w, h)
    one.variance = 1
    one.denoise_resolve = 1
    _frame(one)
    one.denoise()
    spatial = one.denoised()
    one.denoise_temporal()
    s = volren_amd.ShardedRenderer(w, h, [0, 0])
    s.each(lambda p: _configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    assert s.denoise_resolve == 0
    s.denoise_resolve = 1
    assert s.denoise_resolve == 1 and all(p.denoise_resolve == 1 for p in s.parts)
    s.render(SPP)
    s.render_features(2)
    with pytest.raises(volren_amd.VolrenError, match="not last filled by render_features_expected"):
        s.denoise()
    s.render_features_expected(RAYS)
    s.denoise()
    assert _same(s.framebuffer(), one.framebuffer()) and _same(s.features(), one.features())
    assert _same(s.denoised(), spatial) and _same(s.parts[0].resolved(), one.resolved())
    s.denoise_temporal()
    assert _same(s.denoised(), one.denoised())
    s.close()
    one.close()


def test_volpy_has_the_calls():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.cam_fov = 40.0
    vr.render(4)
    vr.render_features_expected(2)
    vr.resolve()
    y = vr.resolved_data()
    assert y.shape == vr.fbo_data().shape == (40, 24, 3) and np.array_equal(y.reshape(-1), vr._r.resolved()[..., :3].reshape(-1))
    assert not np.array_equal(y, vr.fbo_data())
    assert vr.denoise_resolve == 0
    vr.denoise_resolve = 1
    assert vr.denoise_resolve == 1 and vr._r.denoise_resolve == 1


def test_cli_resolve_writes_the_resolved_frame_alone_and_in_front_of_the_filter(tmp_path):
    from PIL import Image

    from oracle import binding as ob
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "6", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    r = scenes.hip_scene("readme", 96, 80)
    r.variance = 1
    r.render(6)
    r.render_features_expected(2)
    r.denoise_resolve = 1
    r.denoise()
    for flags, frame in ((["--resolve"], r.resolved()), (["--denoise", "--resolve"], r.denoised())):
        out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + flags + ["--expected-features", "2", "--output", "rs.png"], cwd=tmp_path,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        img = np.asarray(Image.open(tmp_path / "rs_000000.png"))
        tm = frame.copy()
        ob.lib().orc_tonemap(ob.fptr(tm), 96, 80, 3.0, 2.0)
        want = np.floor(np.clip(tm[::-1], 0, 1) * 255.0 + 0.5).astype(np.uint8)
        assert img.shape == (80, 96, 4) and np.array_equal(img, want), flags
    r.close()
