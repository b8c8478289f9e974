"""GPU: the one-pass regression ("denoise_filter" = 1: vr_filters.hip denoise_regress_kernel in the place of the a-trous iterations, between the layered
filter's split and merge) bit for bit against the host composition of the same headers (tests/hk_regress.py on tests/hostkernel/regress_host.cpp, itself held
to a float64 statement by tests/test_regress_host.py), on frames with partial tiles and frames thinner than the window; vr_denoise_temporal with rejection and
with moments against the host chain; the setting at 0 against a renderer that never saw it; vr_upsample behind it; every refusal on a live renderer; the
sharded renderer; the volpy and command-line layers."""
import subprocess

import numpy as np
import pytest

import hk_regress as hg
import hk_resolve as hr
import hk_upsample as hu
import scenes
import volren_amd
from gpu_frames import _camera, _orbit
from hk_common import same as _same
from test_gpu_resolve import _configure, _frame, _pair
from test_regress_capi import check_settings

pytestmark = pytest.mark.gpu

W, H, SPP, RAYS = 64, 48, 4, 2                  # 4 x 3 tiles
SCENES = ("c2", "c3env", "c3", "c4_64")          # smoke.brick in front of the sky; under the LUT with the sky shown; under the LUT as configured (sky hidden); dense fp16
RIDGES = (hg.default_ridge(), 1.0)               # the default (zero order) and a first-order fit, which runs the solve


def _on(r, ridge=None):
    r.variance = 1
    r.denoise_layers = 1
    r.denoise_filter = 1
    if ridge is not None:
        r.denoise_ridge = ridge


def _host(r, o):
    """the host composition on the renderer's own buffers: (out, L, y, S)"""
    fb, feat = r.framebuffer(), r.features()
    y, B = hr.resolved(o, RAYS, fb, feat)
    out, L, S, _ = hg.layered(y, B, feat, r.denoise_ridge, r.denoise_iterations, tuple(r.denoise_sigma))
    return out, L, y, S


@pytest.mark.parametrize("ridge", RIDGES)
@pytest.mark.parametrize("name", SCENES)
def test_the_whole_call_matches_the_host_bit_for_bit(name, ridge):
    """a 64x48 frame of 4 spp against 2 x 2 expected rays: vr_denoised and vr_denoised_layer after vr_denoise; every pixel without coverage is the background;
    with zero iterations the merge of the split alone; the variance, the framebuffer and the features are left as they were"""
    r, o = _pair(name, W, H)
    _on(r, ridge)
    _frame(r)
    fb, feat, var = r.framebuffer(), r.features(), r.variance()
    r.denoise()
    out, L, _, S = _host(r, o)
    assert _same(r.denoised(), out) and _same(r.denoised_layer(), L)
    assert _same(r.framebuffer(), fb) and _same(r.features(), feat) and _same(r.variance(), var)
    assert _same(out[..., 3], feat[..., 3]) and _same(L[..., 3], feat[..., 3]) and np.isfinite(out).all()
    none = feat[..., 3] == 0
    assert none.sum() > 100 or name == "c4_64"
    assert _same(out[none][:, :3], r.resolve_background()[none][:, :3]) and not np.abs(L[none]).any()
    covered = feat[..., 3] > 0.5
    assert covered.sum() > 50 and not _same(L[covered][:, :3], S[covered][:, :3])      # (the layer was filtered)
    r.denoise_iterations = 0
    r.denoise()
    out0, L0, _, _ = _host(r, o)
    assert _same(r.denoised(), out0) and _same(r.denoised_layer(), L0) and _same(L0[..., :3], S[..., :3])
    r.close()


def test_the_two_ridges_and_the_atrous_differ():
    r, o = _pair("c4_64", W, H)
    _on(r)
    _frame(r)
    seen = []
    for flt, ridge in ((0, 0.0), (1, 0.0), (1, 1.0), (1, 2.0 ** -20)):
        r.denoise_filter, r.denoise_ridge = flt, ridge
        r.denoise()
        seen.append(r.denoised())
        if flt:
            assert _same(seen[-1], _host(r, o)[0])
    assert all(not _same(a, b) for i, a in enumerate(seen) for b in seen[:i])
    r.close()


# thin both ways, one pixel past a tile, one short of two tiles: the window's halo lies outside the frame on every side
@pytest.mark.parametrize("w,h", ((1, 37), (37, 1), (17, 16), (33, 31)))
def test_thin_and_one_past_a_tile_frames_match_the_host_bit_for_bit(w, h):
    r, o = _pair("c2", w, h)
    _on(r)
    _frame(r, spp=2)
    for ridge in RIDGES:
        r.denoise_ridge = ridge
        r.denoise()
        out, L, _, _ = _host(r, o)
        assert _same(r.denoised(), out) and _same(r.denoised_layer(), L), ridge
    r.close()


@pytest.mark.parametrize("setting,value", (("denoise_reject", 3.0), ("denoise_moments", 1)))
def test_three_temporal_frames_match_the_host_chain(setting, value):
    """c3env, three frames of 4 spp, the camera turned 1 degree per frame about the volume, a first-order fit: history (which holds the unfiltered layer), result
    and layer"""
    r, o = _pair("c3env", W, H)
    _on(r, 1.0)
    setattr(r, setting, value)
    replay = hg.Replay(moments=setting == "denoise_moments")
    for i in range(3):
        for x in (r, o):
            _orbit(x, 1.0 * i)
        _frame(r, seed=100 + i)
        r.denoise_temporal()
        fb, feat = r.framebuffer(), r.features()
        y, B = hr.resolved(o, RAYS, fb, feat)
        want = replay.frame(_camera(r), y, B, r.variance(), feat, r.sample, r.denoise_alpha, r.denoise_ridge, r.denoise_iterations, tuple(r.denoise_sigma),
                            tau=r.denoise_reject)
        hc, hv, hn = r.denoise_history()
        for got, ref, part in ((hc, want[0], "C"), (hv, want[1], "V"), (hn, want[2], "N"), (r.denoised(), want[3], "denoised"), (r.denoised_layer(), want[4], "L")):
            assert _same(got, ref), (setting, i, part)
    assert (hn == 3).mean() > 0.5
    r.close()


def test_the_setting_at_0_is_a_renderer_that_never_heard_of_it():
    """denoised, the layer, the history and the framebuffer after the setting went 1 and back to 0, against a fresh renderer's"""
    a, _ = _pair("c3env", W, H)
    b, _ = _pair("c3env", W, H)
    for r in (a, b):
        r.variance = 1
        r.denoise_layers = 1
    _frame(b)
    b.denoise_filter = 1
    b.denoise_ridge = 1.0
    b.denoise()
    b.denoise_temporal()
    b.denoise_filter = 0
    with pytest.raises(volren_amd.VolrenError, match="no history"):      # the change dropped it
        b.denoise_history()
    for r in (a, b):
        _frame(r, seed=7)
        r.denoise()
    assert _same(a.denoised(), b.denoised()) and _same(a.denoised_layer(), b.denoised_layer()) and _same(a.framebuffer(), b.framebuffer())
    for i in range(2):
        for r in (a, b):
            _frame(r, seed=8 + i)
            r.denoise_temporal()
        assert _same(a.denoised(), b.denoised()) and _same(a.denoised_layer(), b.denoised_layer())
        for x, y in zip(a.denoise_history(), b.denoise_history()):
            assert _same(x, y)
    a.close()
    b.close()


def test_upsample_after_a_regression_call_is_the_host_upsample_of_the_host_layer():
    from oracle import binding as ob
    w, h, f = 36, 28, 2
    r, o = _pair("c3env", w, h)
    _on(r, 1.0)
    _frame(r)
    r.denoise()
    _, L, _, _ = _host(r, o)
    assert _same(r.denoised_layer(), L)
    r.upsample(f, RAYS)
    out, Lh, fh, _ = hu.chain(L, r.features(), _configure(ob.OracleRenderer(f * w, f * h), "c3env", True), RAYS, f, tuple(r.denoise_sigma))
    assert _same(r.upsampled_features(), fh) and _same(r.upsampled(), out) and _same(r.upsampled_layer(), Lh)
    r.close()


def test_every_refusal_on_a_live_renderer():
    """the settings' values; the calls without denoise_layers = 1, and with it whatever it refuses -- each VR_ERR with its reason, before a launch: the last result
    stays.  A change of the setting drops the history, either way."""
    r, _ = _pair("c3env", 48, 40)
    check_settings(r)
    r.variance = 1
    _frame(r)
    r.denoise()
    plain = r.denoised()
    r.denoise_filter = 1

    def refused(words):
        for call in (r.denoise, r.denoise_temporal):
            with pytest.raises(volren_amd.VolrenError, match=words):
                call()

    refused("denoise_filter = 1 needs denoise_layers = 1")
    assert _same(r.denoised(), plain)
    r.denoise_layers = 1
    r.denoise()
    good, layer = r.denoised(), r.denoised_layer()
    r.render_features(4)
    refused("denoise_layers = 1: the feature buffer was not last filled by render_features_expected")
    r.render_features_expected(1)
    refused("denoise_layers = 1: the expected-value pass ran with rays = 1; rays >= 2 is needed")
    r.render_features_expected(2)
    r.set_tiles([0, 1])
    refused("tile subset")
    r.set_tiles([])
    r.integrator = 2
    refused("denoise_layers = 1: integrator = 2")
    r.integrator = 0
    assert _same(r.denoised(), good) and _same(r.denoised_layer(), layer)
    for v in (0, 1):
        r.denoise_temporal()
        assert (r.denoise_history()[2] == 1).all()
        r.denoise_filter = v
        with pytest.raises(volren_amd.VolrenError, match="no history"):
            r.denoise_history()
    r.denoise_temporal()
    r.denoise_filter = 1                             # no change: the history stays
    r.denoise_ridge = 0.5                            # nor does the ridge touch it: the history holds the unfiltered layer
    assert (r.denoise_history()[2] == 1).all()
    r.close()


def test_two_logical_shards_equal_one_device():
    name, w, h = "c3env", 96, 64
    one, _ = _pair(name, w, h)
    _on(one, 1.0)
    _frame(one)
    one.denoise()
    spatial, layer = one.denoised(), one.denoised_layer()
    one.denoise_temporal()
    s = volren_amd.ShardedRenderer(w, h, [0, 0])
    s.each(lambda p: _configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    assert s.denoise_filter == 0 and s.denoise_ridge == hg.default_ridge()
    s.denoise_filter = 1
    s.denoise_ridge = 1.0
    assert s.denoise_filter == 1 and all(p.denoise_filter == 1 and p.denoise_ridge == 1.0 for p in s.parts)
    s.render(SPP)
    s.render_features_expected(RAYS)
    with pytest.raises(volren_amd.VolrenError, match="denoise_filter = 1 needs denoise_layers = 1"):
        s.denoise()
    s.denoise_layers = 1
    s.denoise()
    assert _same(s.framebuffer(), one.framebuffer()) and _same(s.features(), one.features())
    assert _same(s.denoised(), spatial) and _same(s.denoised_layer(), layer)
    s.denoise_temporal()
    assert _same(s.denoised(), one.denoised()) and _same(s.denoised_layer(), one.denoised_layer())
    s.close()
    one.close()


def test_the_volpy_and_cli_paths_write_the_same_png(tmp_path):
    from PIL import Image

    import volren_amd.volpy as volpy
    from oracle import binding as ob
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "6", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    r = scenes.hip_scene("readme", 96, 80)
    r.variance = 1
    r.denoise_layers = 1
    r.render(6)
    r.render_features_expected(2)
    images = []
    for flags, flt, ridge in (([], 0, None), (["--denoise-filter", "1"], 1, None), (["--denoise-filter", "1", "--denoise-ridge", "0.5"], 1, 0.5)):
        r.denoise_filter = flt
        if ridge is not None:
            r.denoise_ridge = ridge
        r.denoise()
        out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--denoise", "--denoise-layers", "--expected-features", "2"] + flags + ["--output", "rg.png"],
                             cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        img = np.asarray(Image.open(tmp_path / "rg_000000.png"))
        tm = r.denoised()
        ob.lib().orc_tonemap(ob.fptr(tm), 96, 80, 3.0, 2.0)
        want = np.floor(np.clip(tm[::-1], 0, 1) * 255.0 + 0.5).astype(np.uint8)
        assert img.shape == (80, 96, 4) and np.array_equal(img, want), flags
        images.append(img.copy())
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])
    # volpy: the names pass through to the inner renderer, and its frame is that renderer's
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.cam_fov = 40.0
    vr.variance = 1
    vr.denoise_layers = 1
    vr.render(4)
    vr.render_features_expected(2)
    vr.denoise()
    atrous = vr.denoised_data()
    assert vr.denoise_filter == 0 and vr.denoise_ridge == hg.default_ridge()
    vr.denoise_filter = 1
    vr.denoise_ridge = 0.5
    assert vr.denoise_filter == 1 and vr._r.denoise_filter == 1 and vr._r.denoise_ridge == 0.5
    vr.denoise()
    data = vr.denoised_data()
    assert not np.array_equal(data, atrous) and np.array_equal(data.reshape(-1), vr._r.denoised()[..., :data.shape[-1]].reshape(-1))
    r.close()
