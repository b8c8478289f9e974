"""GPU: vr_upsample (vr_filters.hip upsample_kernel behind an expected-value pass at the upsampled size) bit for bit against the host build of the same
headers (tests/hk_upsample.py on tests/hostkernel/upsample_host.cpp, itself held to a float64 statement by tests/test_upsample_host.py), on frames whose
hi and lo sizes are no multiples of the tile; the hi feature buffer against a renderer of that size; after vr_denoise_temporal; a renderer that never
makes the call; every refusal on a live renderer; the sharded renderer's part 0; the volpy and command-line layers."""
import subprocess

import numpy as np
import pytest

import hk_layers as hl
import hk_resolve as hr
import hk_upsample as hu
import scenes
import volren_amd
from gpu_frames import _camera, _orbit
from hk_common import same as _same
from test_gpu_layers import _host as _host_lo
from test_gpu_resolve import _configure, _frame, _pair

pytestmark = pytest.mark.gpu

SPP, RAYS = 4, 2
SCENES = ("c2", "c3env", "c3", "c4_64")          # smoke.brick in front of the sky; under the LUT with the sky shown; under the LUT as configured (sky hidden); dense fp16
# lo size and factor: hi frames of 72x56, 72x57 and 72x56 -- 5 x 4 tiles, the last column and the top row partial, and lo sizes that are no multiple of the tile
SHAPES = ((36, 28, 2), (24, 19, 3), (18, 14, 4))


def _oracle_hi(name, w, h, f):
    from oracle import binding as ob
    return _configure(ob.OracleRenderer(f * w, f * h), name, True)


def _layered(r):
    r.variance = 1
    r.denoise_layers = 1
    _frame(r, SPP)
    r.denoise()


def _check(r, o_hi, f, rays=RAYS):
    """r.upsample(f, rays) against the host chain fed with the renderer's own layer and lo features; -> (out, L, hi features, B)"""
    L, feat = r.denoised_layer(), r.features()
    r.upsample(f, rays)
    assert r.upsampled_size() == (f * r.width, f * r.height)
    out, Lh, fh, B = hu.chain(L, feat, o_hi, rays, f, tuple(r.denoise_sigma))
    assert _same(r.upsampled_features(), fh)
    assert _same(r.upsampled(), out) and _same(r.upsampled_layer(), Lh)
    assert _same(out[..., 3], fh[..., 3]) and _same(Lh[..., 3], fh[..., 3])
    return out, Lh, fh, B


@pytest.mark.parametrize("w,h,f", SHAPES)
@pytest.mark.parametrize("name", SCENES)
def test_the_frame_the_layer_and_the_hi_features_match_the_host_bit_for_bit(name, w, h, f):
    r, o = _pair(name, w, h)
    _layered(r)
    _, L_lo, _, _ = _host_lo(r, o)
    assert _same(r.denoised_layer(), L_lo)                               # (the lo chain is the host's too)
    out, Lh, fh, B = _check(r, _oracle_hi(name, w, h, f), f)
    none = fh[..., 3] == 0
    if name != "c4_64":
        assert none.sum() > 100
    assert _same(out[none][:, :3], B[none][:, :3]) and not np.abs(Lh[none]).any()      # kappa_p = 0: the background itself
    assert np.isfinite(out).all() and (out[..., :3] >= 0).all()
    covered = fh[..., 3] > 0.5
    assert covered.sum() > 50 and np.abs(Lh[covered][:, :3]).max() > 1e-3              # (the layer did arrive at the hi size)
    if name == "c3":
        assert not B.any()
    r.close()


@pytest.mark.parametrize("w,h", ((1, 37), (37, 1)))
def test_thin_frames_match_the_host_bit_for_bit(w, h):
    r, _ = _pair("c2", w, h)
    r.variance = 1
    r.denoise_layers = 1
    _frame(r, spp=2)
    r.denoise()
    _check(r, _oracle_hi("c2", w, h, 2), 2)
    r.close()


def test_the_hi_features_are_those_of_a_renderer_of_that_size_and_the_lo_renderer_is_left_as_it_was():
    """c3env, lo 24x19, f = 3, 3 x 3 rays: vr_upsampled_features against vr_render_features_expected of a second renderer resized to 72x57, with and without
    the clear-distance table; the lo framebuffer, features, vr_denoised, vr_denoised_layer and the history before and after the call; and a renderer that
    never makes the call computes the same next frames."""
    a, _ = _pair("c3env", 24, 19)
    b, _ = _pair("c3env", 24, 19)
    big, _ = _pair("c3env", 16, 16)
    big.resize(72, 57)
    big.render_features_expected(3)
    want = big.features()
    for r in (a, b):
        r.variance = 1
        r.denoise_layers = 1
        _frame(r, SPP)
        r.denoise_temporal()
    before = (b.framebuffer(), b.features(), b.denoised(), b.denoised_layer(), b.variance()) + tuple(b.denoise_history())
    b.upsample(3, 3)
    assert _same(b.upsampled_features(), want)
    b.expected_skip = 0
    b.expected_stats(True)
    b.upsample(3, 3)
    assert _same(b.upsampled_features(), want)
    big.expected_skip = 0
    big.expected_stats(True)
    big.render_features_expected(3)
    stats = b.expected_stats()
    assert stats == big.expected_stats() and stats["rays"] > 24 * 19 * 9 and stats["reads"] == 0      # the hi pass's own work was counted, and it read no table
    b.expected_skip = 1
    b.expected_stats(False)
    after = (b.framebuffer(), b.features(), b.denoised(), b.denoised_layer(), b.variance()) + tuple(b.denoise_history())
    for x, y in zip(before, after):
        assert _same(x, y)
    for i in range(2):
        for r in (a, b):
            _frame(r, SPP, seed=50 + i)
            r.denoise_temporal()
        assert _same(a.denoised(), b.denoised()) and _same(a.denoised_layer(), b.denoised_layer()) and _same(a.features(), b.features())
        for x, y in zip(a.denoise_history(), b.denoise_history()):
            assert _same(x, y)
    with pytest.raises(volren_amd.VolrenError, match="no upsample since the last resize"):
        a.upsampled()
    for r in (a, b, big):
        r.close()


def test_after_three_temporal_frames_under_a_turning_camera():
    """c3env, lo 36x28, f = 2, three frames of 4 spp, the camera turned 1 degree per frame about the volume: the lo chain is the host's (hk_layers.Replay),
    and vr_upsample after every vr_denoise_temporal is the host chain's on that layer with the hi scene under the same camera"""
    w, h, f = 36, 28, 2
    r, o = _pair("c3env", w, h)
    o_hi = _oracle_hi("c3env", w, h, f)
    r.variance = 1
    r.denoise_layers = 1
    replay = hl.Replay()
    for i in range(3):
        for x in (r, o, o_hi):
            _orbit(x, 1.0 * i)
        _frame(r, SPP, seed=100 + i)
        r.denoise_temporal()
        fb, guide = r.framebuffer(), r.features()
        y, B = hr.resolved(o, RAYS, fb, guide)
        want = replay.frame(_camera(r), y, B, r.variance(), guide, r.sample, r.denoise_alpha, r.denoise_iterations, tuple(r.denoise_sigma))
        assert _same(r.denoised_layer(), want[4]), i
        r.upsample(f, RAYS)
        out, Lh, fh, _ = hu.chain(want[4], guide, o_hi, RAYS, f, tuple(r.denoise_sigma))
        assert _same(r.upsampled_features(), fh) and _same(r.upsampled(), out) and _same(r.upsampled_layer(), Lh), i
    assert (r.denoise_history()[2] >= 2).mean() > 0.5
    r.close()


def test_every_refusal_on_a_live_renderer():
    """no layer yet, a layer of before the resize, a tile subset, arguments out of range: each with its code and reason, before a launch -- the last result
    stays; the read-backs before the first call and after a resize; a call with another factor reallocates"""
    lib = volren_amd.load()
    r, o = _pair("c2", 20, 12)
    r.variance = 1
    for call in (r.upsampled, r.upsampled_layer, r.upsampled_features, r.upsampled_size):
        with pytest.raises(volren_amd.VolrenError, match="no upsample since the last resize"):
            call()
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1 since the last resize"):
        r.upsample()
    _frame(r, SPP)
    r.denoise()                                                          # denoise_layers = 0: still no layer
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1 since the last resize"):
        r.upsample(2, 2)
    r.denoise_layers = 1
    r.denoise()
    for factor, rays, words in ((1, 2, b"factor must be 2..4"), (5, 2, b"factor must be 2..4"), (2, 0, b"rays must be 1..4"), (2, 5, b"rays must be 1..4")):
        assert lib.vr_upsample(r._h, factor, rays) == 3 and words in lib.vr_last_error()      # VR_ERR_ARG
    r.upsample()                                                         # factor 2, 2 x 2 rays
    assert r.upsampled_size() == (40, 24)
    good, layer, feats = r.upsampled(), r.upsampled_layer(), r.upsampled_features()
    assert good.shape == (24, 40, 4) and layer.shape == (24, 40, 4) and feats.shape == (24, 40, 8)
    r.set_tiles([0])
    assert lib.vr_upsample(r._h, 2, 2) == 1 and b"tile subset" in lib.vr_last_error()         # VR_ERR
    r.set_tiles([])
    assert _same(r.upsampled(), good) and _same(r.upsampled_layer(), layer) and _same(r.upsampled_features(), feats)
    r.upsample(3, 1)                                                     # another factor: other buffers
    assert r.upsampled_size() == (60, 36) and r.upsampled().shape == (36, 60, 4) and r.upsampled_features().shape == (36, 60, 8)
    out, Lh, fh, _ = hu.chain(r.denoised_layer(), r.features(), _oracle_hi("c2", 20, 12, 3), 1, 3, tuple(r.denoise_sigma))
    assert _same(r.upsampled(), out) and _same(r.upsampled_layer(), Lh) and _same(r.upsampled_features(), fh)
    r.upsample(2, 2)
    assert _same(r.upsampled(), good) and _same(r.upsampled_layer(), layer)
    r.resize(12, 20)
    for call in (r.upsampled, r.upsampled_layer, r.upsampled_features, r.upsampled_size):
        with pytest.raises(volren_amd.VolrenError, match="no upsample since the last resize"):
            call()
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1 since the last resize"):
        r.upsample(2, 2)
    r.close()


def test_part_0_of_two_logical_shards_equals_one_device():
    name, w, h, f = "c3env", 48, 40, 2
    one, _ = _pair(name, w, h)
    _layered(one)
    one.upsample(f, RAYS)
    s = volren_amd.ShardedRenderer(w, h, [0, 0])
    s.each(lambda p: _configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    s.denoise_layers = 1
    s.render(SPP)
    s.render_features_expected(RAYS)
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1"):
        s.parts[0].upsample(f, RAYS)
    s.denoise()
    assert _same(s.denoised_layer(), one.denoised_layer())
    s.parts[0].upsample(f, RAYS)
    assert s.parts[0].upsampled_size() == (f * w, f * h)
    assert _same(s.parts[0].upsampled(), one.upsampled()) and _same(s.parts[0].upsampled_layer(), one.upsampled_layer())
    assert _same(s.parts[0].upsampled_features(), one.upsampled_features())
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1"):      # a part that holds no gathered layer
        s.parts[1].upsample(f, RAYS)
    s.close()
    one.close()


def test_volpy_has_the_names():
    import volren_amd.volpy as volpy
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
    vr.upsample()
    data = vr.upsampled_data()
    assert data.shape == (80, 48, 3) and np.array_equal(data.reshape(-1), vr._r.upsampled()[..., :3].reshape(-1))
    vr.upsample(factor=3, rays=1)
    assert vr.upsampled_data().shape == (120, 72, 3)


def test_cli_flag_writes_the_large_frame_and_is_refused_alone(tmp_path):
    from PIL import Image

    from oracle import binding as ob
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "48", "-h", "40", "--render", "--spp", "6", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    r = scenes.hip_scene("readme", 48, 40)
    r.variance = 1
    r.denoise_layers = 1
    r.render(6)
    r.render_features_expected(2)
    r.denoise()
    r.upsample(2, 2)
    out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--denoise", "--denoise-layers", "--expected-features", "2", "--upsample", "2", "--output", "up.png"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    img = np.asarray(Image.open(tmp_path / "up_000000.png"))
    tm = r.upsampled()
    ob.lib().orc_tonemap(ob.fptr(tm), 96, 80, 3.0, 2.0)
    want = np.floor(np.clip(tm[::-1], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert img.shape == (80, 96, 4) and np.array_equal(img, want)
    out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--upsample", "2", "--output", "no.png"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "--upsample needs --denoise-layers" in out.stderr
    r.close()
