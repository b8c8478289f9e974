"""GPU: albedo demodulation ("denoise_demodulate" = 1: the DEMOD instances of vr_filters.hip's layers_split_kernel, denoise_prepare_kernel,
layers_merge_kernel and upsample_kernel) bit for bit against the host composition of the same headers (tests/hk_demod.py on
tests/hostkernel/demod_host.cpp, itself held to a float64 statement by tests/test_demod_host.py), through the public calls: vr_denoise under both filters,
vr_denoise_temporal plain, with rejection and with moments, vr_upsample on layers made with and without the setting, the sharded renderer; the refusals,
the dropped history, and the setting at 0 against a renderer that never saw it."""
import numpy as np
import pytest

import hk_demod as hd
import hk_layers as hl
import hk_resolve as hr
import hk_upsample as hu
import volren_amd
from gpu_frames import _camera, _orbit
from hk_common import same as _same
from test_demod_capi import check_setting
from test_gpu_resolve import _configure, _frame, _pair

pytestmark = pytest.mark.gpu

SPP, RAYS = 4, 2
SIZES = ((64, 48), (37, 21))                     # 4 x 3 whole tiles; a size no tile divides
SCENES = ("c3", "c3env")                         # under the LUT as configured (sky hidden); with the sky shown


def _on(r, ridge=None):
    r.variance = 1
    r.denoise_layers = 1
    r.denoise_demodulate = 1
    r.denoise_filter = 0 if ridge is None else 1
    if ridge is not None:
        r.denoise_ridge = ridge


def _host(r, o, ridge=None):
    """the host composition on the renderer's own buffers: (out, L, S, F)"""
    fb, feat = r.framebuffer(), r.features()
    y, B = hr.resolved(o, RAYS, fb, feat)
    return hd.layered(y, B, r.variance(), feat, r.sample, r.denoise_iterations, tuple(r.denoise_sigma), ridge)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_denoise_matches_the_host_bit_for_bit(name, w, h):
    """a frame of 4 spp against 2 x 2 expected rays: vr_denoised and vr_denoised_layer after vr_denoise at 0, 1 and 5 iterations and under "denoise_filter" 1
    at ridge 0 and 0.01; every pixel without coverage that the filter's footprint carried coverage onto is the background; the variance, the framebuffer and the features are left as they were; the result is
    not the plain layered call's"""
    r, o = _pair(name, w, h)
    _on(r)
    _frame(r)
    fb, feat, var = r.framebuffer(), r.features(), r.variance()
    none = feat[..., 3] == 0
    for n in (0, 1, 5):
        r.denoise_iterations = n
        r.denoise()
        out, L, S, F = _host(r, o)
        assert _same(r.denoised(), out) and _same(r.denoised_layer(), L), n
        hit = none & (F[..., 3] > hl.MIN_WEIGHT)
        assert _same(out[hit][:, :3], r.resolve_background()[hit][:, :3]) and not np.abs(L[hit]).any()
    assert hit.sum() > 100
    y, B = hr.resolved(o, RAYS, fb, feat)
    assert not _same(out, hl.layered(y, B, var, feat, SPP)[0]) and not _same(S, hl.split(y, B, feat[..., 3]))
    for ridge in (0.0, 0.01):
        _on(r, ridge)
        r.denoise()
        out, L, _, _ = _host(r, o, ridge)
        assert _same(r.denoised(), out) and _same(r.denoised_layer(), L), ridge
    assert _same(r.framebuffer(), fb) and _same(r.features(), feat) and _same(r.variance(), var)
    assert _same(out[..., 3], feat[..., 3]) and np.isfinite(out).all()
    r.close()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("mode", ("plain", "reject", "moments"))
def test_three_temporal_frames_match_the_host_chain(mode, name, w, h):
    """three frames with the camera turned 1 degree per frame about the volume -- 4 spp, with "denoise_reject" 3, or 1 spp with "denoise_moments": the
    history (which holds the demodulated layer), the result and the layer"""
    r, o = _pair(name, w, h)
    _on(r)
    if mode == "reject":
        r.denoise_reject = 3.0
    if mode == "moments":
        r.denoise_moments = 1
    replay = hd.Replay(moments=mode == "moments")
    for i in range(3):
        for x in (r, o):
            _orbit(x, 1.0 * i)
        _frame(r, spp=1 if mode == "moments" else SPP, seed=100 + i)
        r.denoise_temporal()
        fb, feat = r.framebuffer(), r.features()
        y, B = hr.resolved(o, RAYS, fb, feat)
        want = replay.frame(_camera(r), y, B, r.variance(), feat, r.sample, r.denoise_alpha, r.denoise_iterations, tuple(r.denoise_sigma), tau=r.denoise_reject)
        hc, hv, hn = r.denoise_history()
        for got, ref, part in ((hc, want[0], "C"), (hv, want[1], "V"), (hn, want[2], "N"), (r.denoised(), want[3], "denoised"), (r.denoised_layer(), want[4], "L")):
            assert _same(got, ref), (mode, name, i, part)
    if mode != "moments":
        assert not _same(hc, hl.split(y, B, feat[..., 3]))       # (not the plain layer's history)
    assert (hn == 3).any()                               # (histories did accumulate)
    r.close()


@pytest.mark.parametrize("made_with", (1, 0))
@pytest.mark.parametrize("f", (2, 3))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_upsample_demodulates_whatever_made_the_layer(name, w, h, f, made_with):
    """lo 64x48 (whole tiles, lo and hi) and 37x21 (no tile divides it, nor the hi frame's), with the sky hidden (G = 0, no environment lookup) and shown: the lo layer of a call with the setting or without it, then vr_upsample with the setting 1
    against the host chain on that layer; with the setting 0 at the call it is today's"""
    from oracle import binding as ob
    r, o = _pair(name, w, h)
    _on(r)
    r.denoise_demodulate = made_with
    _frame(r)
    r.denoise()
    L = r.denoised_layer()
    r.denoise_demodulate = 1
    r.upsample(f, RAYS)
    o_hi = _configure(ob.OracleRenderer(f * w, f * h), name, True)
    out, Lh, fh, _ = hd.chain(L, r.features(), o_hi, RAYS, f, tuple(r.denoise_sigma))
    assert _same(r.upsampled_features(), fh) and _same(r.upsampled(), out) and _same(r.upsampled_layer(), Lh)
    assert _same(r.denoised_layer(), L)
    r.denoise_demodulate = 0
    r.upsample(f, RAYS)
    plain, Lp, _, _ = hu.chain(L, r.features(), o_hi, RAYS, f, tuple(r.denoise_sigma))
    assert _same(r.upsampled(), plain) and _same(r.upsampled_layer(), Lp) and not _same(plain, out)
    r.close()


@pytest.mark.parametrize("name", SCENES)
def test_two_logical_shards_equal_one_device(name):
    w, h = 64, 48
    one, _ = _pair(name, w, h)
    _on(one)
    _frame(one)
    one.denoise()
    spatial, layer = one.denoised(), one.denoised_layer()
    one.denoise_temporal()
    s = volren_amd.ShardedRenderer(w, h, [0, 0])
    s.each(lambda p: _configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    assert s.denoise_demodulate == 0
    s.denoise_demodulate = 1
    assert s.denoise_demodulate == 1 and all(p.denoise_demodulate == 1 for p in s.parts)
    s.render(SPP)
    s.render_features_expected(RAYS)
    with pytest.raises(volren_amd.VolrenError, match="denoise_demodulate = 1 needs denoise_layers = 1"):
        s.denoise()
    s.denoise_layers = 1
    s.denoise()
    assert _same(s.framebuffer(), one.framebuffer()) and _same(s.features(), one.features())
    assert _same(s.denoised(), spatial) and _same(s.denoised_layer(), layer)
    s.denoise_temporal()
    assert _same(s.denoised(), one.denoised()) and _same(s.denoised_layer(), one.denoised_layer())
    s.close()
    one.close()


def test_the_refusals_launch_nothing_and_a_change_drops_the_history():
    """the setting's values; the calls without denoise_layers = 1 -- VR_ERR with the reason, before a launch: the last result stays readable and as it was.
    A change of the setting drops the history, either way; setting the value it has does not."""
    r, _ = _pair("c3env", 48, 40)
    check_setting(r)
    r.variance = 1
    _frame(r)
    r.denoise()
    plain = r.denoised()
    r.denoise_demodulate = 1
    for call in (r.denoise, r.denoise_temporal):
        with pytest.raises(volren_amd.VolrenError, match="denoise_demodulate = 1 needs denoise_layers = 1"):
            call()
    assert _same(r.denoised(), plain)
    r.denoise_layers = 1
    r.denoise()
    good, layer = r.denoised(), r.denoised_layer()
    assert not _same(good, plain)
    r.set_tiles([0, 1])
    for call in (r.denoise, r.denoise_temporal):
        with pytest.raises(volren_amd.VolrenError, match="tile subset"):
            call()
    r.set_tiles([])
    assert _same(r.denoised(), good) and _same(r.denoised_layer(), layer)
    for v in (0, 1):
        r.denoise_temporal()
        assert (r.denoise_history()[2] == 1).all()
        r.denoise_demodulate = v
        with pytest.raises(volren_amd.VolrenError, match="no history"):
            r.denoise_history()
    r.denoise_temporal()
    r.denoise_demodulate = 1                         # no change: the history stays
    assert (r.denoise_history()[2] == 1).all()
    r.close()


def test_the_setting_at_0_is_a_renderer_that_never_heard_of_it():
    """denoised, the layer, the history, the upsampled frame and the framebuffer after the setting went 1 and back to 0, against a fresh renderer's"""
    a, _ = _pair("c3env", 37, 21)
    b, _ = _pair("c3env", 37, 21)
    for r in (a, b):
        r.variance = 1
        r.denoise_layers = 1
    _frame(b)
    b.denoise_demodulate = 1
    b.denoise()
    b.denoise_temporal()
    b.upsample(2, RAYS)
    b.denoise_demodulate = 0
    for r in (a, b):
        _frame(r, seed=7)
        r.denoise()
        r.upsample(2, RAYS)
    assert _same(a.denoised(), b.denoised()) and _same(a.denoised_layer(), b.denoised_layer()) and _same(a.framebuffer(), b.framebuffer())
    assert _same(a.upsampled(), b.upsampled()) and _same(a.upsampled_layer(), b.upsampled_layer())
    for i in range(2):
        for r in (a, b):
            _frame(r, seed=8 + i)
            r.denoise_temporal()
        assert _same(a.denoised(), b.denoised()) and _same(a.denoised_layer(), b.denoised_layer())
        for x, y in zip(a.denoise_history(), b.denoise_history()):
            assert _same(x, y)
    a.close()
    b.close()
