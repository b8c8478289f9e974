"""GPU: every image-space kernel of vr_filters.hip, one launcher at a time through vr_filter_probe, on the crafted frames of tests/filter_cases.py against the
host build of the same header, bit for bit -- the frames tests/test_filter_cases_host.py holds to the float64 statements on the CPU first: zero and over-unit
normals, depth 0, colours from 1e-6 to 1e5, subnormal and overflowing variances, reprojections onto the frame's edge and behind the camera, histories of 2^20
frames, singular regression windows, NaN and inf texels; and, with demod = 1, the DEMOD instances of vr_demod.h on albedo words at and around the floor, above 1,
negative, subnormal, NaN and inf.  Then three chains in which the device is fed its own outputs stage by stage (the third demodulated), and vr_denoise on a
rendered frame reproduced by the probe's prepare and atrous from the renderer's read-backs -- and, demodulated, on a ragged frame through split, prepare with
counts, atrous and merge: the hook runs the product's launches."""
import numpy as np
import pytest

import filter_cases as fc
import scenes
import volren_amd
from hk_common import same as _same

pytestmark = pytest.mark.gpu


def _hip(scene, w, h):
    """the device twin of filter_cases.oracle: c3env = c3 with the sky shown, c2hid = c2 with it hidden"""
    r = scenes.hip_scene({"c3env": "c3", "c2hid": "c2"}.get(scene, scene), w, h)
    if scene == "c3env":
        r.show_environment = 1
    if scene == "c2hid":
        r.show_environment = 0
    return r


class _Renderers:
    """one small renderer per scene and size, made on demand and closed together"""

    def __init__(self):
        self.made = {}

    def get(self, scene, w, h):
        if (scene, w, h) not in self.made:
            self.made[(scene, w, h)] = _hip(scene, w, h)
        return self.made[(scene, w, h)]

    def close(self):
        for r in self.made.values():
            r.close()


def _compare(case, got, want):
    """the differences of a case's outputs, as messages"""
    assert set(got) == set(want), (case.id, sorted(got), sorted(want))
    return [m for m in (fc.first_difference(case, name, got[name], want[name]) for name in sorted(want)) if m]


@pytest.mark.parametrize("group", sorted(fc.GROUPS))
def test_the_kernel_equals_the_host_build_on_every_case(group):
    """bit for bit; in a non-finite case a NaN may be any NaN, at the same place.  The scene-free stages run on one 16x16 renderer of c2, whatever the case's
    size; resolve and upsample on a renderer of the case's scene and size."""
    rs = _Renderers()
    bad = []
    try:
        for c in fc.cases(group):
            r = rs.get(c.scene, c.w, c.h) if c.scene else rs.get("c2", 16, 16)
            bad += _compare(c, fc.device(r, c), fc.host(c))
    finally:
        rs.close()
    assert not bad, "%d outputs differ\n%s" % (len(bad), "\n".join(bad[:8]))


def test_the_scene_bound_stages_refuse_a_size_that_is_not_the_renderers_and_the_renderer_is_left_as_it_was():
    r = _hip("c2", 17, 16)
    r.variance = 1
    r.render(2)
    r.render_features_expected(2)
    r.denoise_layers = 1
    r.denoise_temporal()
    before = (r.framebuffer(), r.features(), r.denoised(), r.denoised_layer(), r.variance()) + tuple(r.denoise_history())
    c = next(x for x in fc.cases("resolve") if (x.scene, x.w, x.h) == ("c2", 17, 16))
    assert not _compare(c, fc.device(r, c), fc.host(c))
    wrong = fc.Case("resolve", "wrong-size", 16, 16, {"fb": np.zeros((16, 16, 4), np.float32), "feat": np.zeros((16, 16, 8), np.float32)}, {"rays": 2}, scene="c2")
    with pytest.raises(volren_amd.VolrenError, match="resolution"):
        fc.device(r, wrong)
    up = next(x for x in fc.cases("upsample") if (x.scene, x.w, x.h) == ("c2", 17, 16))
    assert not _compare(up, fc.device(r, up), fc.host(up))
    for c in fc.cases("temporal-reject")[:3] + fc.cases("temporal-moments")[:3] + fc.cases("regress")[:2]:
        assert not _compare(c, fc.device(r, c), fc.host(c))
    after = (r.framebuffer(), r.features(), r.denoised(), r.denoised_layer(), r.variance()) + tuple(r.denoise_history())
    assert all(_same(a, b) for a, b in zip(before, after))
    r.denoise_temporal()                                     # the history is still there, and the call continues it: lengths 2 where there was one
    assert (r.denoise_history()[2] == 2).sum() > 50
    r.close()


def _chain_step(r, stage, name, w, h, dev_in, host_in, par=None, scene=None):
    """the device fed the device's own outputs, the host the host's"""
    d = fc.device(r, fc.Case(stage, name, w, h, dev_in, par, scene=scene))
    return d, fc._HOST[stage](fc.Case(stage, name, w, h, host_in, par, scene=scene))


def test_the_atrous_chain_fed_its_own_outputs():
    """prepare, temporal (a 1 degree orbit over a history), five a-trous steps on the hostile frame: each stage of the device reads what the device's stage before
    it wrote, and the end equals the host chain bit for bit.  (Were a stage off by a bit the stages behind it would show it compounded; the per-stage test above
    says which.)"""
    col, S, feat = fc.frame()
    tc = next(x for x in fc.cases("temporal-plain") if x.name == "plain-orbit-1deg")
    r = _hip("c2", 16, 16)
    w, h = fc.W0, fc.H0
    d, q = _chain_step(r, "prepare", "chain", w, h, {"S": S, "feat": feat}, {"S": S, "feat": feat}, {"n": 8})
    par = dict(tc.par)
    d2, q2 = _chain_step(r, "temporal", "chain", w, h, {"color": col, "v": d["v"], "guide": d["guide"], "hist": tc.inp["hist"]},
                         {"color": col, "v": q["v"], "guide": q["guide"], "hist": tc.inp["hist"]}, par)
    dc, dv, qc, qv = d2["color"], d2["v"], q2["color"], q2["v"]
    assert (q2["record"][..., 1] > 1).sum() > 100
    for k in range(5):
        par = {"step": 1 << k, "sigma": fc.SIGMA, "vout": k < 4}
        da, qa = _chain_step(r, "atrous", "chain%d" % k, w, h, {"color": dc, "v": dv, "guide": d["guide"]}, {"color": qc, "v": qv, "guide": q["guide"]}, par)
        dc, qc = da["color"], qa["color"]
        if k < 4:
            dv, qv = da["v"], qa["v"]
    r.close()
    end = fc.Case("atrous", "chain-end", w, h, {"color": col, "guide": q["guide"]})
    msg = fc.first_difference(end, "color", dc, qc)
    assert msg is None, msg
    assert np.isfinite(qc).all() and not _same(qc, col)


def test_the_regression_chain_fed_its_own_outputs():
    """resolve, split, prepare, temporal, regress, merge, upsample on c2 at 17x16, upsampled by 2: the device's stages feed each other, and the upsampled frame and
    layer equal the host chain's bit for bit"""
    w, h, f = 17, 16, 2
    rc = next(x for x in fc.cases("resolve") if (x.scene, x.w, x.h) == ("c2", w, h))
    uc = next(x for x in fc.cases("upsample") if (x.scene, x.w, x.h, x.par["f"]) == ("c2", w, h, f))
    _, S0, _ = fc.frame(w, h, seed=13)
    fb, feat = rc.inp["fb"], rc.inp["feat"]
    r = _hip("c2", w, h)
    d, q = _chain_step(r, "resolve", "chain", w, h, rc.inp, rc.inp, rc.par, scene="c2")
    ds, qs = _chain_step(r, "split", "chain", w, h, {"y": d["y"], "B": d["B"], "feat": feat}, {"y": q["y"], "B": q["B"], "feat": feat})
    dp, qp = _chain_step(r, "prepare", "chain", w, h, {"S": S0, "feat": feat}, {"S": S0, "feat": feat}, {"n": 4})
    cur = fc.orbit_camera(11.0, height=0.3)
    hist = fc.history(np.random.default_rng(77), cur, fc.orbit_camera(10.0, height=0.25), np.ascontiguousarray(qp["guide"][..., 3]), np.ascontiguousarray(qp["guide"][..., 7]), w, h, False)
    par = {"cur": fc.f32(cur), "alpha": 0.1, "tau": 0.0, "form": "plain", "sigma": fc.SIGMA}
    dt, qt = _chain_step(r, "temporal", "chain", w, h, {"color": ds["S"], "v": dp["v"], "guide": dp["guide"], "hist": hist},
                         {"color": qs["S"], "v": qp["v"], "guide": qp["guide"], "hist": hist}, par)
    assert (qt["record"][..., 1] > 1).sum() > 20
    par = {"ridge": 0.01, "sigma": fc.SIGMA}
    dr, qr = _chain_step(r, "regress", "chain", w, h, {"S": dt["color"], "guide": dp["guide"]}, {"S": qt["color"], "guide": qp["guide"]}, par)
    dm, qm = _chain_step(r, "merge", "chain", w, h, {"F": dr["F"], "B": d["B"], "feat": feat}, {"F": qr["F"], "B": q["B"], "feat": feat})
    du, qu = _chain_step(r, "upsample", "chain", w, h, {"L": dm["L"], "glo": dp["guide"], "feat_hi": uc.inp["feat_hi"]},
                         {"L": qm["L"], "glo": qp["guide"], "feat_hi": uc.inp["feat_hi"]}, uc.par, scene="c2")
    r.close()
    end = fc.Case("upsample", "chain-end", w, h, {})
    bad = _compare(end, du, qu)
    assert not bad, "\n".join(bad)
    assert np.isfinite(qu["out"]).all() and np.abs(qu["L"][..., :3]).max() > 1e-3 and not _same(qm["out"], fb)


def test_the_demodulated_chain_fed_its_own_outputs():
    """the regression chain again on c3env at 17x16, upsampled by 2, with demod = 1 in split, prepare, merge and upsample and the albedo words of the lo features
    drawn from the catalogue's finite ALBEDOS (the hi features are the catalogue's demodulated upsample case's): the history, the regression and the taps read the
    divided layer the device's own split wrote, and the end equals the host chain bit for bit"""
    w, h, f = 17, 16, 2
    rc = next(x for x in fc.cases("resolve") if (x.scene, x.w, x.h) == ("c2", w, h))                 # (its frame and coverage, under c3env's sky)
    uc = next(x for x in fc.cases("demod") if x.stage == "upsample" and (x.scene, x.w, x.h, x.par["f"]) == ("c3env", w, h, f))
    _, S0, _ = fc.frame(w, h, seed=13)
    fb, feat = rc.inp["fb"], rc.inp["feat"].copy()
    feat[..., 0:3] = np.random.default_rng(78).choice(fc.ALBEDOS, (h, w, 3))
    demod = {"demod": 1}
    r = _hip("c3env", w, h)
    d, q = _chain_step(r, "resolve", "demod-chain", w, h, {"fb": fb, "feat": feat}, {"fb": fb, "feat": feat}, rc.par, scene="c3env")
    ds, qs = _chain_step(r, "split", "demod-chain", w, h, {"y": d["y"], "B": d["B"], "feat": feat}, {"y": q["y"], "B": q["B"], "feat": feat}, demod)
    dp, qp = _chain_step(r, "prepare", "demod-chain", w, h, {"S": S0, "feat": feat}, {"S": S0, "feat": feat}, {"n": 4, "demod": 1})
    cur = fc.orbit_camera(11.0, height=0.3)
    hist = fc.history(np.random.default_rng(77), cur, fc.orbit_camera(10.0, height=0.25), np.ascontiguousarray(qp["guide"][..., 3]), np.ascontiguousarray(qp["guide"][..., 7]), w, h, False)
    par = {"cur": fc.f32(cur), "alpha": 0.1, "tau": 0.0, "form": "plain", "sigma": fc.SIGMA}
    dt, qt = _chain_step(r, "temporal", "demod-chain", w, h, {"color": ds["S"], "v": dp["v"], "guide": dp["guide"], "hist": hist},
                         {"color": qs["S"], "v": qp["v"], "guide": qp["guide"], "hist": hist}, par)
    assert (qt["record"][..., 1] > 1).sum() > 20
    par = {"ridge": 0.01, "sigma": fc.SIGMA}
    dr, qr = _chain_step(r, "regress", "demod-chain", w, h, {"S": dt["color"], "guide": dp["guide"]}, {"S": qt["color"], "guide": qp["guide"]}, par)
    dm, qm = _chain_step(r, "merge", "demod-chain", w, h, {"F": dr["F"], "B": d["B"], "feat": feat}, {"F": qr["F"], "B": q["B"], "feat": feat}, demod)
    du, qu = _chain_step(r, "upsample", "demod-chain", w, h, {"L": dm["L"], "glo": dp["guide"], "feat_hi": uc.inp["feat_hi"]},
                         {"L": qm["L"], "glo": qp["guide"], "feat_hi": uc.inp["feat_hi"]}, uc.par, scene="c3env")
    r.close()
    end = fc.Case("upsample", "demod-chain-end", w, h, {})
    bad = _compare(end, du, qu) + _compare(end, dm, qm)
    assert not bad, "\n".join(bad)
    assert uc.par["demod"] == 1 and np.isfinite(qu["out"]).all() and np.abs(qu["L"][..., :3]).max() > 1e-3
    plain = fc._HOST["merge"](fc.Case("merge", "plain", w, h, {"F": qr["F"], "B": q["B"], "feat": feat}))
    assert not _same(qm["L"], plain["L"]) and not _same(qs["S"], fc._HOST["split"](fc.Case("split", "plain", w, h, {"y": q["y"], "B": q["B"], "feat": feat}))["S"])


def _moments_behind(var, n_px):
    """vr_variance is the moments times float(n) / float(n - 1) of the pixel's tile, and prepare with counts forms that very product again: moments that give
    the read-back's words bit for bit, by division and a search over the quotient's neighbours (the true moments are among them or give the same product)"""
    scale = np.array([[fc.variance_scale(int(n)) for n in row] for row in n_px], np.float32)[..., None]
    m = (var / scale).astype(np.float32)
    found = (m * scale).astype(np.float32) == var
    for towards in (np.inf, -np.inf):
        cand = m.copy()
        for _ in range(2):
            cand = np.nextafter(cand, np.float32(towards))
            hit = ~found & ((cand * scale).astype(np.float32) == var)
            m, found = np.where(hit, cand, m), found | hit
    assert found.all(), int((~found).sum())
    return m


def test_the_probe_reproduces_a_demodulated_vr_denoise_of_a_ragged_frame():
    """c3env at 33x31 after render_adaptive(2, 8, a threshold between the tiles' errors): vr_denoise with denoise_layers and denoise_demodulate, then the probe's
    split, prepare with the renderer's tile_samples() as counts, five a-trous steps and merge, all with demod = 1, fed vr_resolved, vr_resolve_background,
    vr_variance and vr_features: vr_denoised and vr_denoised_layer bit for bit.  denoise_prepare_kernel<true> reads counts[q.tile] here and nowhere else."""
    import hk_adaptive
    w, h = 33, 31
    r = _hip("c3env", w, h)
    r.variance = 1
    r.render(2)
    e = np.unique(r.tile_error())
    e = e[np.isfinite(e)]
    r.render_adaptive(2, 8, float(0.5 * (e[len(e) // 2 - 1] + e[len(e) // 2])))
    counts = r.tile_samples()
    assert len(np.unique(counts)) >= 2 and counts.min() >= 2
    r.render_features_expected(2)
    r.denoise_layers = 1
    r.denoise_demodulate = 1
    r.denoise()
    want, want_layer = r.denoised(), r.denoised_layer()
    y, B, var, feat = r.resolved(), r.resolve_background(), r.variance(), r.features()
    n_px = hk_adaptive.per_pixel(counts, w, h)
    px = (h, w, 4)
    S = r.filter_probe("split", w, h, [y, B, feat], [px], demod=True)[0]
    n = int(counts.max())
    v, g = r.filter_probe("prepare", w, h, [_moments_behind(var, n_px), feat, np.ascontiguousarray(counts.reshape(-1), np.int32)], [(h, w), (h, w, 8)], i0=n,
                          x=fc.variance_scale(n), demod=True)
    sigma = tuple(r.denoise_sigma)
    assert r.denoise_iterations == 5
    c = S
    for k in range(5):
        c, v = r.filter_probe("atrous", w, h, [c, v, g], [px, (h, w) if k < 4 else None], sigma=sigma, i0=1 << k)
    out, L = r.filter_probe("merge", w, h, [c, B, feat], [px, px], demod=True)
    assert _same(out, want) and _same(L, want_layer) and not _same(want, r.framebuffer())
    plain = r.filter_probe("merge", w, h, [c, B, feat], [px, px])[1]
    assert not _same(plain, want_layer)                                          # (and the plain instances do not give it)
    assert _same(r.denoised(), want) and _same(r.denoised_layer(), want_layer)
    r.close()


def test_demod_is_refused_outside_0_and_1_and_at_a_stage_without_a_demod_instance():
    r = _hip("c2", 16, 16)
    z4, z8, z1 = np.zeros((16, 16, 4), np.float32), np.zeros((16, 16, 8), np.float32), np.zeros((16, 16), np.float32)
    with pytest.raises(volren_amd.VolrenError, match="demod must be 0 or 1"):
        r.filter_probe("split", 16, 16, [z4, z4, z8], [(16, 16, 4)], demod=2)
    with pytest.raises(volren_amd.VolrenError, match="demod = 1 goes with prepare, split, merge and upsample only"):
        r.filter_probe("atrous", 16, 16, [z4, z1, z8], [(16, 16, 4), (16, 16)], i0=1, demod=True)
    with pytest.raises(volren_amd.VolrenError, match="demod = 1 goes with prepare, split, merge and upsample only"):
        r.filter_probe("regress", 16, 16, [z4, z8], [(16, 16, 4)], demod=True)
    assert not r.filter_probe("split", 16, 16, [z4, z4, z8], [(16, 16, 4)], demod=True)[0].any()      # and the renderer still answers
    r.close()


def test_the_probe_reproduces_vr_denoise_from_the_renderers_read_backs():
    """a rendered 33x31 frame of c2, 4 spp: prepare and five a-trous steps through the probe, fed vr_framebuffer, vr_variance and vr_features, give vr_denoised bit
    for bit.  vr_variance is the moments times n / (n - 1), the product prepare forms itself: handed in as moments with a scale of 1 it is the same float32 number."""
    w, h, n = 33, 31, 4
    r = scenes.hip_scene("c2", w, h)
    r.variance = 1
    r.render(n)
    r.render_features(n)
    r.denoise()
    want = r.denoised()
    fb, var, feat = r.framebuffer(), r.variance(), r.features()
    v, g = r.filter_probe("prepare", w, h, [var, feat, None], [(h, w), (h, w, 8)], i0=n, x=1.0)
    c = fb
    sigma = tuple(r.denoise_sigma)
    iterations = r.denoise_iterations
    assert iterations == 5
    for k in range(iterations):
        c, v = r.filter_probe("atrous", w, h, [c, v, g], [(h, w, 4), (h, w) if k < iterations - 1 else None], sigma=sigma, i0=1 << k)
    assert _same(c, want) and not _same(want, fb)
    assert _same(r.denoised(), want) and _same(r.framebuffer(), fb)
    r.close()
