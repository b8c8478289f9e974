"""CPU: every case of tests/filter_cases.py through the host build of its stage -- range-checked, and under the undefined-behaviour sanitizer, where hk_temporal
and hk_moments offer it -- held to the stage's float64 statement at the tolerance the stage's own host test uses, and to the conditions that make the case worth
running: how many pixels have a history, were rejected, took one, two or four taps, dropped a column.  tests/test_gpu_filter_probe.py then compares the kernels with
these same host results bit for bit; no case reaches a device before it passes here.

Non-finite cases are not compared with float64; they are held to the containment the headers state.  The group "demod" (the DEMOD instances of vr_demod.h) is
held to hk_demod's float64 statements at bounds derived from the header's operation counts, not recorded ones; its overflow cases are compared on their finite
words, and its NaN and inf albedo words must stay in their own channel."""
import numpy as np
import pytest

import filter_cases as fc
import hk_adaptive as ha
import hk_demod as hd
import hk_denoise
import hk_layers as hl
import hk_moments as hm
import hk_regress as hg
import hk_resolve as hr
import hk_temporal as ht
import hk_upsample as hu
import test_layers_host
import test_regress_host
import test_resolve_host
import test_upsample_host
from hk_common import same as _same
from test_adaptive_host import _close as _close_adaptive
from test_denoise_host import _close
from test_moments_host import _close as _close_kept

SUBNORMAL = np.float32(2.0 ** -126)


def _ids(group):
    return [c.name for c in fc.cases(group)]


def _recorded(table, row):
    """the largest recorded |host - float64| of a row of a host test's RECORDED table over its scenes, asserted at 4 x there and here"""
    return 4.0 * max(max(v[row]) for v in table.values())


def _scaled(bound, magnitude, measured_below=2.0):
    """A RECORDED bound of a host test, extended to values larger than the ones it was measured on.  The tables of test_resolve_host, test_layers_host,
    test_regress_host and test_upsample_host are absolute errors of a few float32 roundings of values below `measured_below` (2 for the frames and layers of
    resolve and regress, 4 for the sums of split and merge, as their docstrings say).  A rounding error is relative, so for values up to `magnitude` the bound
    is taken times magnitude / measured_below, and never below the table's own: bound * max(1, magnitude / measured_below).  This factor is this file's; the
    tables say so where they stand."""
    return bound * max(1.0, float(magnitude) / measured_below)


def test_the_catalogue_holds_what_the_kernels_may_be_handed():
    """every group has cases; names are unique; features, guides, cameras and history records are finite, coverage in [0, 1], depth >= 0; a non-finite value
    appears only in a case that says so, and only in a colour, a layer, a moment or a variance"""
    seen = set()
    for group in fc.GROUPS:
        cs = fc.cases(group)
        assert cs, group
        for c in cs:
            assert c.id not in seen, c.id
            seen.add(c.id)
            assert c.w * c.h <= fc.MAX_PIXELS
            for key, a in c.inp.items():
                if a is None:
                    continue
                if key in ("feat", "guide", "glo", "feat_hi"):
                    fourth = key == "feat" and c.nonfinite and c.par.get("demod") == 1 and c.stage in ("prepare", "split", "merge")
                    if fourth:                           # the fourth kind: a NaN or +inf albedo word of a per-pixel DEMOD stage, and no other word of the features
                        assert group == "demod" and not np.isneginf(a).any()
                    assert np.isfinite(a[..., 3:] if fourth else a).all() and (a[..., 3] >= 0).all() and (a[..., 3] <= 1).all() and (a[..., 7] >= 0).all(), (c.id, key)
                elif key == "hist":
                    assert np.isfinite(a[0]).all() and np.isfinite(a[2]).all() and (a[2][..., 1] >= 0).all() and (a[2][..., 3] >= 0).all(), c.id
                    assert all(np.isfinite(p).all() for p in a[1:]), c.id
                elif key in ("tiles", "counts"):
                    assert a.dtype == np.int32
                elif not (c.nonfinite and key in ("S", "color", "v")):
                    assert np.isfinite(a).all(), (c.id, key)
            if "cur" in c.par:
                assert np.isfinite(c.par["cur"]).all()
    assert len(seen) > 150


# ---- prepare ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("prepare"))
def test_prepare(name):
    c = next(x for x in fc.cases("prepare") if x.name == name)
    out = fc.host(c)
    v, g = out["v"], out["guide"]
    S, feat, counts, n = c.inp["S"], c.inp["feat"], c.inp.get("counts"), c.par["n"]
    n_px = np.full((c.h, c.w), n) if counts is None else ha.per_pixel(counts, c.w, c.h)
    assert np.abs(g - hk_denoise.spec_prepare(np.zeros_like(S), feat, 1)[1]).max() <= 1e-6
    covered = feat[..., 3] > 0
    assert (covered & (feat[..., 7] == 0)).any() and (covered & ~feat[..., 4:7].any(axis=-1)).any()      # depth 0 and a zero normal on covered pixels
    assert (v[n_px < 2] == 0).all()
    with np.errstate(all="ignore"):
        scale = np.where(n_px >= 2, n_px / np.maximum(n_px - 1.0, 1.0), 0.0).astype(np.float32)
        var = np.where((n_px >= 2)[..., None], S * scale[..., None], np.float32(0.0))
    if c.nonfinite:
        over = np.isinf(var[..., :3]).any(axis=-1)                               # 3e38 * n / (n - 1) overflows
        assert over.sum() > 100 and np.isposinf(v[over]).all() and np.isfinite(v[~over]).all() and not np.isnan(v).any()
        return
    _close(v, hk_denoise.spec_prepare(var, feat, 1)[0] / n_px, c.id)
    if name.startswith("tiny"):
        assert ((var > 0) & (var < SUBNORMAL)).sum() > 100                      # subnormal variances in ...
        assert ((v > 0) & (v < SUBNORMAL)).sum() > 100, c.id                     # ... and subnormal v out, not flushed
    if counts is not None:
        assert (counts == 1).any() and len(set(counts.reshape(-1).tolist())) >= 6 and (n_px == 1).sum() > 100


# ---- atrous -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("atrous"))
def test_atrous(name):
    c = next(x for x in fc.cases("atrous") if x.name == name)
    out = fc.host(c)
    col, v, g, step, sigma = c.inp["color"], c.inp["v"], c.inp["guide"], c.par["step"], c.par["sigma"]
    assert ("v" in out) == c.par["vout"]
    assert not _same(out["color"], col)
    if c.nonfinite:
        # a colour texel that is not finite reaches the pixels whose 5 x 5 taps at this step hold it (its weight may underflow to 0: then 0 * inf = NaN
        # all the same); an inf variance reaches them through the colour weight's 3 x 3 prefilter and its own term.  Far from both, the case's twin without
        # them gives the same bits.
        bad = ~np.isfinite(col).all(axis=-1) | ~np.isfinite(v)
        clean = fc.host(next(x for x in fc.cases("atrous") if x.name == "step%d" % step))
        reach = np.zeros_like(bad)
        r = 2 * step + 1
        for y, x in np.argwhere(bad):
            reach[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
        assert bad.any() and (~reach).sum() > 100 and _same(out["color"][~reach], clean["color"][~reach])
        hit = ~np.isfinite(col).all(axis=-1)
        assert not hit.any() or not np.isfinite(out["color"][hit]).all(axis=-1).any()
        return
    assert all(np.isfinite(a).all() for a in out.values()), c.id
    if c.ill:
        tol = 1e-6 * np.abs(col).reshape(-1, 4).max(axis=0)
        assert ((out["color"] >= col.reshape(-1, 4).min(axis=0) - tol) & (out["color"] <= col.reshape(-1, 4).max(axis=0) + tol)).all()      # convex combinations
        return
    sc, sv = hk_denoise.spec_atrous(col, v, g, step, sigma)
    _close(out["color"], sc, (c.id, "colour"))
    if c.par["vout"]:
        _close(out["v"], sv, (c.id, "variance"))
    if step == 16 and (c.w, c.h) == (fc.W0, fc.H0):
        y, x = np.mgrid[0:c.h, 0:c.w]
        assert ((x - 32 < 0) & (x + 32 >= c.w) & (y - 32 < 0) & (y + 32 >= c.h)).any()       # pixels whose outer taps leave the frame on every side


# ---- temporal ---------------------------------------------------------------------------------------------------------------------------------------------
def _temporal_facts(c, out):
    """from the host build alone: (has a history [H][W], taps inside the frame [H][W] (0 without reprojection))"""
    i, p = c.inp, c.par
    g = i["guide"]
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    N = out["record"][..., 1]
    hist = i["hist"]
    if hist is None:
        return N > 1, np.zeros((c.h, c.w), int), None
    if hist[0].tobytes() == p["cur"].tobytes():
        return N > 1, np.full((c.h, c.w), 1), None
    u, w, dp, ok = ht.reproject(p["cur"], hist[0], k, d)
    return N > 1, fc.taps_inside(u, w, ok, c.w, c.h), (u, w, dp, ok)


def _temporal_common(c, out):
    """what every form's cases are held to; -> (has, taps, given)"""
    has, taps, given = _temporal_facts(c, out)
    name = c.name.split("-", 1)[1]
    big = (c.w, c.h) == (fc.W0, fc.H0)
    if c.inp["hist"] is None or name == "turned-180":
        assert not has.any() and (out["record"][..., 1] == 1).all(), c.id
        if name == "turned-180":
            assert not given[3].any()                                            # everything behind the history's camera
    elif big and name not in ("one-covered-pixel-history", "tau-0.000976562"):
        assert has.sum() > 100 and (~has).sum() > 50, (c.id, int(has.sum()))
    if name.startswith("translated"):
        u, w, _, ok = given
        band = ok & (((u >= -1) & (u < 0)) | ((u >= c.w - 1) & (u < c.w)))
        assert band.sum() >= 20, (c.id, int(band.sum()))
        for n in (1, 2, 4):
            assert (taps == n).sum() >= 2 and (has & (taps == n)).any(), (c.id, n, int((taps == n).sum()))
    if name in ("orbit-1deg", "fov"):
        assert (taps == 4).sum() > 500
    if c.inp["hist"] is not None and big and not name.startswith(("depth", "n3", "one-covered")):
        N = c.inp["hist"][2][..., 1]
        for n in (0.0, 1.0, 2.0 ** 20):
            assert (N == n).sum() > 50
        K, k = c.inp["hist"][2][..., 2], c.inp["guide"][..., 3]
        assert ((K == 0) & (k > 0)).sum() > 20 and ((K > 0) & (k == 0)).sum() > 5
    if name == "depth-bound":
        x = np.arange(c.w)[None, :] % 3
        live = (c.inp["guide"][..., 3] > 0) & (c.inp["guide"][..., 7] > 0)
        got = [has[live & (x == j)].mean() for j in range(3)]
        # D = d / 0.9 rounded: |D - d| against 0.1 D is rounding's to decide pixel by pixel; one ulp above it no pixel keeps its history, one ulp below every one does
        assert live.sum() > 1000 and got[1] == 0.0 and got[2] == 1.0 and 0.1 < got[0] < 0.9, (c.id, got)
    return has, taps, given


def _near_bound(c, given, alpha):
    i, p = c.inp, c.par
    g = i["guide"]
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    hist = i["hist"][:3]
    res = ht.spec_step(p["cur"], np.zeros((c.h, c.w, 4)), np.zeros((c.h, c.w)), k, d, alpha, hist, given=given)
    with np.errstate(invalid="ignore"):
        return (np.abs(res[5] - ht.DEPTH_BOUND) <= 1e-5).any(axis=-1)


@pytest.mark.parametrize("name", _ids("temporal-plain"))
def test_temporal_plain(name):
    c = next(x for x in fc.cases("temporal-plain") if x.name == name)
    out = fc.host(c)
    i, p = c.inp, c.par
    g = i["guide"]
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    has, taps, given = _temporal_common(c, out)
    C, R = out["color"], out["record"]
    assert _same(R[..., 2], k) and _same(R[..., 3], d) and _same(out["v"], R[..., 0])
    assert _same(C[~has], i["color"][~has]) and _same(R[..., 0][~has], i["v"][~has])
    if c.nonfinite:
        bad = ~np.isfinite(i["color"]).all(axis=-1)
        assert bad.sum() == 8 and has[bad].any() and np.isfinite(C[~bad]).all() and not np.isfinite(C[bad]).all(axis=-1).any()      # the frame's texel reaches its own pixel alone
        return
    assert np.isfinite(C).all() and np.isfinite(R).all()
    if i["hist"] is None:
        return
    sC, sV, sN = ht.spec_step(p["cur"], i["color"], i["v"], k, d, p["alpha"], i["hist"], given=given)[:3]
    keep = ~_near_bound(c, given, p["alpha"])
    if not name.endswith("depth-bound"):
        assert (~keep).mean() <= 0.01
    assert np.array_equal(R[..., 1][keep], sN[keep].astype(np.float32))
    assert np.allclose(C[keep], sC[keep], rtol=1e-5, atol=1e-30) and np.allclose(R[..., 0][keep], sV[keep], rtol=1e-5, atol=1e-30)
    if name.endswith("alpha-1"):
        assert np.allclose(C[..., :3], i["color"][..., :3], rtol=1e-6, atol=0) and (R[..., 1][has] >= 2).all()
    if name.endswith("same-camera"):
        assert (R[..., 1] == 2.0 ** 20).sum() > 20                             # the cap: 2^20 - 1 and 2^20 both end there


@pytest.mark.parametrize("name", _ids("temporal-reject"))
def test_temporal_reject(name):
    c = next(x for x in fc.cases("temporal-reject") if x.name == name)
    out = fc.host(c)
    i, p = c.inp, c.par
    g = i["guide"]
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    C, R, T = out["color"], out["record"], out["T"]
    had = T != np.float32(ht.NO_HISTORY)                                         # had a history before the decision
    rej = ht.rejected(T, p["tau"])
    has, taps, given = _temporal_common(c, {"record": np.where(had[..., None], np.float32(2), np.float32(1)) * np.ones(4, np.float32)})
    keep = had & ~rej
    assert _same(R[..., 2], k) and _same(R[..., 3], d) and _same(out["v"], R[..., 0])
    assert (R[..., 1][~keep] == 1).all() and _same(C[~keep], i["color"][~keep]) and _same(R[..., 0][~keep], i["v"][~keep])
    tag = name.split("-", 1)[1]
    big = (c.w, c.h) == (fc.W0, fc.H0)
    if c.nonfinite:
        bad = ~np.isfinite(i["color"]).all(axis=-1)
        near = np.zeros_like(bad)
        for y, x in np.argwhere(bad):
            near[max(0, y - 2):y + 3, max(0, x - 2):x + 3] = True
        assert np.isfinite(T[~near]).all() and (~np.isfinite(T[near & had])).any()      # the statistic pools a 5 x 5 window: a NaN z2 stays inside it ...
        assert rej[near & had & ~np.isfinite(T)].all()                                   # ... and rejects
        return
    assert np.isfinite(C).all() and np.isfinite(R).all() and np.isfinite(T).all()
    if i["hist"] is None or tag == "turned-180":
        assert not had.any()
        return
    if tag == "tau-0.000976562":
        assert had.sum() > 100 and rej[had].mean() > 0.99                       # the smallest threshold rejects (all but exact matches)
    elif tag == "tau-1.04858e+06":
        assert keep.sum() > 100 and rej.sum() < 0.5 * had.sum()
    elif tag in ("v0", "v0-both"):
        assert rej[had].mean() > 0.9, (c.id, rej[had].mean())                   # no variance anywhere: every z2 with a difference is (difference)^2 / 1e-12
    elif big and tag not in ("depth-bound",):
        assert keep.sum() > 20 and rej.sum() > 20, (c.id, int(keep.sum()), int(rej.sum()))
    fh, h, vh, nh = ht.spec_fetch(p["cur"], k, d, i["hist"], given=given)
    near_b = _near_bound(c, given, p["alpha"])
    ok = ~near_b
    for dy in range(-2, 3):                                                     # a pixel left out of the fetch is left out of every window that holds it
        for dx in range(-2, 3):
            ok &= ~hk_denoise._shift(near_b.astype(np.float64), dy, dx)[0].astype(bool)
    assert np.array_equal(had[~near_b], fh[~near_b])
    sT = ht.spec_stat(i["color"], i["v"], fh, h, vh)
    cmp_ = ok & had & fh
    assert np.allclose(T[cmp_], sT[cmp_], rtol=1e-5, atol=0), (c.id, np.abs(T[cmp_] / sT[cmp_] - 1).max())
    sC, sV, sN = ht.spec_step(p["cur"], i["color"], i["v"], k, d, p["alpha"], i["hist"], given=given)[:3]
    kk = keep & ~near_b
    assert np.array_equal(R[..., 1][kk], sN[kk].astype(np.float32))
    assert np.allclose(C[kk], sC[kk], rtol=1e-5, atol=1e-30) and np.allclose(R[..., 0][kk], sV[kk], rtol=1e-5, atol=1e-30)


@pytest.mark.parametrize("name", _ids("temporal-moments"))
def test_temporal_moments(name):
    c = next(x for x in fc.cases("temporal-moments") if x.name == name)
    out = fc.host(c)
    i, p = c.inp, c.par
    g = i["guide"]
    k, d = np.ascontiguousarray(g[..., 3]), np.ascontiguousarray(g[..., 7])
    C, R, M = out["color"], out["record"], out["moments"]
    has, taps, given = _temporal_common(c, out)
    assert _same(R[..., 2], k) and _same(R[..., 3], d) and _same(out["v"], R[..., 0])
    tag = name.split("-", 1)[1]
    if c.nonfinite:
        bad = ~np.isfinite(i["color"]).all(axis=-1)
        near = np.zeros_like(bad)
        for y, x in np.argwhere(bad):
            near[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = True
        assert np.isfinite(M[~near]).all() and np.isfinite(R[~near]).all() and not np.isfinite(M[bad][:, :2]).all(axis=-1).any()      # pass 2 pools a 7 x 7 window
        return
    assert np.isfinite(C).all() and np.isfinite(R).all() and np.isfinite(M).all() and (M[..., 3] >= 0).all()
    C1, R1, M1 = hm.pass1(p["cur"], i["color"], k, d, p["alpha"], i["hist"], checked=True)
    sC, sN, s1, s2, sE, near = hm.spec_pass1(p["cur"], i["color"], k, d, p["alpha"], i["hist"], given=given)
    keep = ~near
    assert np.array_equal(R1[..., 1][keep], sN[keep].astype(np.float32))
    assert _close_kept(C1, sC, keep) and _close_kept(M1[..., 0], s1, keep) and _close_kept(M1[..., 1], s2, keep) and _close_kept(M1[..., 2], sE, keep)
    S, V, a2 = hm.spec_pass2(g, p["sigma"], R1[..., 1], M1[..., 0], M1[..., 1], M1[..., 2])
    assert (np.abs(M[..., 3] - S) <= 1e-5 * a2).all() and (np.abs(R[..., 0] - V) <= 1e-5 * a2 * M1[..., 2]).all()
    solid = S >= 0.01 * a2
    assert np.allclose(M[..., 3][solid], S[solid], rtol=1e-3, atol=0) and np.allclose(R[..., 0][solid], V[solid], rtol=1e-3, atol=0)
    if tag == "n3-n4-clamped":
        N = R[..., 1]
        assert {3.0, 4.0} <= set(np.unique(N).tolist()) <= {1.0, 3.0, 4.0}
        long_ = N == 4
        assert (M[..., 3][long_] == 0).sum() > 50 and (M[..., 3][long_] > 0).sum() > 50      # m2 - m1^2 of either sign by rounding: clamped, and not
        assert (M[..., 3][N == 3] > 0).mean() > 0.9                                            # the short histories pool their window instead
    elif tag.startswith("one-covered-pixel"):
        assert (k > 0).sum() == 1
    elif i["hist"] is not None and (c.w, c.h) == (fc.W0, fc.H0) and tag not in ("turned-180", "depth-bound"):
        assert ((R[..., 1] >= 4) & has).sum() > 50 and ((R[..., 1] < 4) & has).sum() > 50, c.id


# ---- resolve ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("resolve"))
def test_resolve(name):
    c = next(x for x in fc.cases("resolve") if x.name == name)
    out = fc.host(c)
    fb, kappa = c.inp["fb"], c.inp["feat"][..., 3]
    B, y = out["B"], out["y"]
    for a in (0.0, 1.0, None):                          # all nine combinations of the frame's alpha and the expected coverage: 0, 1, a fraction
        for b in (0.0, 1.0, None):
            m = ((fb[..., 3] == a) if a is not None else (fb[..., 3] > 0) & (fb[..., 3] < 1)) & ((kappa == b) if b is not None else (kappa > 0) & (kappa < 1))
            assert m.sum() >= (1 if min(c.w, c.h) == 1 else 10), (c.id, a, b)
    assert np.isfinite(y).all() and _same(y[..., 3], kappa)
    if c.scene == "c2hid":
        assert not B.any()
    else:
        assert (B[..., :3] > 0).all() and not B[..., 3].any()
        assert (np.abs(B[..., :3] - hr.spec_background(fc.oracle(c.scene, c.w, c.h), c.par["rays"])).max() <= _recorded(test_resolve_host.RECORDED, 0))
    # the table's y was measured on oracle frames, whose x, B and pooled C~ = sum P.rgb / sum P.a stay below 2; here a window of few hits under a bright sky gives
    # a larger C~, and y = x + (B - C~)(alpha - kappa) rounds at that magnitude
    P = out["P"].astype(np.float64)
    Sw = hr._window_sum(P)
    Ct = np.where((Sw[..., 3] > 0)[..., None], Sw[..., :3] / np.where(Sw[..., 3] > 0, Sw[..., 3], 1.0)[..., None], 0.0)
    big = max(float(np.abs(B).max()), float(np.abs(Ct).max()), float(np.abs(y).max()))
    assert np.abs(y - hr.spec_resolve(fb, B, kappa))[..., :3].max() <= _scaled(_recorded(test_resolve_host.RECORDED, 1), big)
    assert not _same(y[..., :3], fb[..., :3])


# ---- split / merge ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("layers"))
def test_layers(name):
    c = next(x for x in fc.cases("layers") if x.name == name)
    out = fc.host(c)
    kappa, B = c.inp["feat"][..., 3], c.inp["B"]
    for kv in fc.KAPPAS:
        assert (kappa == kv).sum() > 100
    big = max(float(np.abs(a).max()) for a in list(out.values()) + [B])
    scale = _scaled(1.0, big, 4.0)                       # the tables were measured on values below 4
    if c.stage == "split":
        S = out["S"]
        assert _same(S[..., 3], kappa) and (S[..., :3] < 0).mean() > 0.2 and (S[..., :3] > 0).mean() > 0.2      # y < B: S is signed
        assert np.abs(S - hl.spec_split(c.inp["y"], B, kappa))[..., :3].max() <= _recorded(test_layers_host.RECORDED, 0) * scale
        return
    F = c.inp["F"]
    o, L = out["out"], out["L"]
    so, sl = hl.spec_merge(F, B, kappa)
    assert _same(o[..., 3], kappa) and _same(L[..., 3], kappa) and (o[..., :3] >= 0).all()
    # the ratio kappa / F.a reaches 2^19 where F.a = 2^-19 and kappa = 1: the layer's magnitude is in `scale`
    assert np.abs(o - so)[..., :3].max() <= _recorded(test_layers_host.RECORDED, 1) * scale and np.abs(L - sl)[..., :3].max() <= _recorded(test_layers_host.RECORDED, 2) * scale
    if name == "alpha-is-kappa":
        live = kappa > hl.MIN_WEIGHT
        assert _same(F[..., 3], kappa) and _same(L[..., :3][live], F[..., :3][live])          # the ratio is kappa / kappa = 1
    else:
        assert (F[..., 3] != kappa).mean() > 0.5 and ((F[..., 3] <= hl.MIN_WEIGHT) & (kappa > 0)).sum() > 100 and ((F[..., 3] > hl.MIN_WEIGHT) & (F[..., 3] != kappa)).sum() > 100


# ---- regress ----------------------------------------------------------------------------------------------------------------------------------------------
_DROPS = {}


def _dropped(c):
    """how many columns each pixel dropped (-1: it never reached the solve), by the header's own counter; the counting run gives the filter's bits"""
    if c.id not in _DROPS:
        with np.errstate(all="ignore"):
            F, n = hg.dropped(c.inp["S"], c.inp["guide"], c.par["ridge"], c.par["sigma"])
        want = fc.host(c)["F"]
        assert ((F.view(np.uint32) == want.view(np.uint32)) | (np.isnan(F) & np.isnan(want))).all(), c.id
        _DROPS[c.id] = n
    return _DROPS[c.id]


@pytest.mark.parametrize("name", _ids("regress"))
def test_regress(name):
    c = next(x for x in fc.cases("regress") if x.name == name)
    F = fc.host(c)["F"]
    S, g, ridge = c.inp["S"], c.inp["guide"], c.par["ridge"]
    kp = g[..., 3]
    n = _dropped(c)
    assert _same(F[..., 3], kp) and not F[kp == 0].any()
    kind = name.rsplit("-ridge", 1)[0]
    if c.nonfinite:
        # vr_regress.h: a NaN in S.rgb of a tap that counts makes F NaN in the pixels whose window holds it, and only those (an inf: inf or NaN)
        bad = ~np.isfinite(S).all(axis=-1)
        counts = bad & (S[..., 3] > hg.MIN_WEIGHT) & (kp > 0)
        assert counts.sum() == 2
        reach = np.zeros_like(bad)
        for y, x in np.argwhere(counts):
            reach[max(0, y - 5):y + 6, max(0, x - 5):x + 6] = True
        assert np.isfinite(F[~reach]).all() and not np.isfinite(F[reach & (kp > 0)]).all(axis=-1).any()
        clean = fc.host(next(x for x in fc.cases("regress") if x.name == "albedo-flat-ridge%g" % ridge))["F"]
        assert _same(F[~reach], clean[~reach])
        return
    assert np.isfinite(F).all(), c.id
    if ridge > 0:
        solved = n >= 0
        if kind == "flat":
            assert solved.all() and (n == 0).all()       # every slope column is empty: each pivot is the ridge itself, above the floor, and is kept
        elif kind == "lone":
            assert solved.sum() == (kp > 0).sum() == 12 and (n[solved] == 0).all()
        elif kind == "faint":
            assert not solved.any() and not F[..., :3].any() and (kp > 0).sum() == 12          # A_00 <= 2^-20: F = (0, 0, 0, kappa)
    if kind == "lone":
        at = kp > 0
        assert np.allclose(F[at][:, :3], S[at][:, :3], rtol=1e-6, atol=0)                     # one tap, the centre: C~ = S.rgb / S.a, times kappa = S.a
    if kind == "depth0":
        assert ((kp > 0) & (g[..., 7] == 0)).sum() > 500
    if kind == "checker":
        assert (kp > 0).sum() > 700 and (kp == 0).sum() > 700
    # The float64 statement, every case at every ridge.  The bound per pixel: test_regress_host's RECORDED table at its 4 x (the zero-order row at ridge 0, the
    # first-order row at every ridge above), scaled by the layer's magnitude as _scaled says, plus what vr_regress.h says a kept column costs: the pivot d_k is what
    # is left of the diagonal a_k, and a_k is a sum over up to 121 taps, each addition a rounding of 2^-24 relative -- sqrt(121) = 11 of them as a random walk -- so
    # d_k is off by 11 x 2^-24 a_k and Ct by that times (a_k / d_k - 1) of the magnitude, for each kept slope column.  That is nothing where the ridge carries the
    # pivot, and 2.7e-3 relative at the very edge of the 2^-12 rule.  A pixel where float32 and float64 decide a column differently is left out, and must have that
    # column's share within a factor 2 of 2^-12.
    with np.errstate(all="ignore"):
        want, share, kept = hg.spec(S, g, ridge, c.par["sigma"], detail=True)
    mag = float(np.abs(want[..., :3]).max())
    tol = np.full(kp.shape, _scaled(_recorded(test_regress_host.RECORDED, 0 if ridge == 0 else 1), mag))
    keep = np.ones(kp.shape, bool)
    if ridge > 0:
        tol = tol + 11.0 * 2.0 ** -24 * mag * np.where(kept[..., 1:], 1.0 / share[..., 1:] - 1.0, 0.0).sum(axis=-1)
        other = (n >= 0) & ((~kept).sum(axis=-1) != n)
        edge = ((share > 0.5 * hg.PIVOT_SHARE) & (share < 2.0 * hg.PIVOT_SHARE)).any(axis=-1)
        assert not (other & ~edge).any() and other.mean() <= 0.01, (c.id, int(other.sum()))
        keep = ~other
    err = np.abs(F - want)[..., :3].max(axis=-1)
    assert (err <= tol)[keep].all(), (c.id, float((err / tol)[keep].max()), float(err[keep].max()))
    if kind == "pit" and 0 < ridge <= 1:
        at_pit = (n > 0)
        assert at_pit.sum() > 700 and (share[at_pit][:, 1] < hg.PIVOT_SHARE).all()      # the depth column keeps 2^-20 of its diagonal at most: noise, dropped on both sides


def test_regress_elimination_drops_columns_and_keeps_them():
    """over the catalogue, from the host build alone: some pixel of some case drops a column (a pivot at or below the floor) and some pixel keeps all seven slopes
    next to the intercept; printed per case"""
    some, all_kept = 0, 0
    for c in fc.cases("regress"):
        if c.par["ridge"] == 0 or c.nonfinite:
            continue
        n = _dropped(c)
        live = n >= 0
        print("%-28s solved %4d  kept all %4d  dropped one or more %4d  (most %d)" % (c.name, live.sum(), (n == 0).sum(), (n > 0).sum(), n.max()))
        some += int((n > 0).sum())
        all_kept += int((n == 0).sum())
    assert some > 0 and all_kept > 0, (some, all_kept)


# ---- upsample ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("upsample"))
def test_upsample(name):
    c = next(x for x in fc.cases("upsample") if x.name == name)
    out = fc.host(c)
    f = c.par["f"]
    L, glo = c.inp["L"], c.inp["glo"]
    ghi = hu.guide(c.inp["feat_hi"])
    B, _ = hr.prepare(fc.oracle(c.scene, f * c.w, f * c.h), c.par["rays"], np.zeros((f * c.h, f * c.w, 4), np.float32))
    o, Lh = out["out"], out["L"]
    assert np.isfinite(o).all() and np.isfinite(Lh).all() and (o[..., :3] >= 0).all()
    assert _same(o[..., 3], ghi[..., 3]) and _same(Lh[..., 3], ghi[..., 3])
    rep = np.repeat(np.repeat(glo, f, axis=0), f, axis=1)
    equal = (ghi.view(np.uint32) == rep.view(np.uint32)).all(axis=-1) & (ghi[..., 3] > 0)
    assert equal.sum() >= 5, (c.id, int(equal.sum()))                            # a hi guide equal to the lo tap's under it, bit for bit
    assert ((ghi[..., 3] == 0) & (rep[..., 3] > 0)).sum() >= 2 and ((ghi[..., 3] > 0) & (rep[..., 3] == 0)).sum() >= 1, c.id
    none = ghi[..., 3] == 0
    assert _same(o[none][:, :3], B[none][:, :3]) and not Lh[none].any()
    so, sl, De, Ds = hu.spec_upsample(L, glo, ghi, B, f, c.par["sigma"])
    near = (np.abs(De - hu.MIN_WEIGHT) < 1e-3 * hu.MIN_WEIGHT) | (np.abs(Ds - hu.MIN_WEIGHT) < 1e-3 * hu.MIN_WEIGHT)
    assert near.mean() <= 0.01
    assert np.abs(o - so)[~near][:, :3].max() <= _recorded(test_upsample_host.RECORDED, 0) and np.abs(Lh - sl)[~near][:, :3].max() <= _recorded(test_upsample_host.RECORDED, 1)
    assert (De > hu.MIN_WEIGHT).any() and ((De <= hu.MIN_WEIGHT) & (ghi[..., 3] > 0)).any() or min(c.w, c.h) == 1      # both tiers


# ---- the DEMOD instances (vr_demod.h) -----------------------------------------------------------------------------------------------------------------------
# Every bound below is derived, not recorded: per output word, the number of float32 roundings in vr_demod.h's statement of it, times 2^-24, times the float64 sum
# of the magnitudes of the statement's terms at that pixel (divided or multiplied by d as the statement is), plus 2^-149 for a result in the subnormal range.
#   split    S = (y - (1 - kappa) B) / d: 1 - kappa, its product with B, the difference, the quotient                       4 roundings of (|y| + |1 - kappa| |B|) / d
#   merge    L = (F (kappa / F.a)) d: the ratio, two products                                                              3 roundings of |F| (kappa / F.a) d
#            out = max_(G + L, 0): G's two, L's three, the sum (max_ moves nothing apart)                                  6 roundings of |G| + |L|
#   v        test_demod_host.py's 2^-21, relative, per pixel
#   upsample _upsample_bound below
U = 2.0 ** -24
TINY = 2.0 ** -149
FLT_MAX = float(np.finfo(np.float32).max)
_WORST = {}                                              # stage -> (the largest |host - float64| / bound over the finite cases run so far, the case)


def _note(stage, case, err, bound):
    ratio = float((err / bound).max())
    if ratio > _WORST.get(stage, (0.0, None))[0]:
        _WORST[stage] = (ratio, case.id)
    print("%-34s worst |host - float64| %.3e, %.3f of its derived bound (%.3e there)" % (case.id, float(err.max()), ratio, float(bound.reshape(-1)[np.argmax(err / bound)])))
    return ratio


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _census(feats):
    """how many covered pixels hold each value of ALBEDOS (bit for bit: the two zeros apart) in some channel, over the feature buffers of a case"""
    return [sum(int(((_bits(f[..., 0:3]) == _bits(a)).any(axis=-1) & (f[..., 3] > 0)).sum()) for f in feats) for a in fc.ALBEDOS]


def _plain_twin(c):
    """the case with demod 0, through the catalogue's own dispatch"""
    return fc._HOST[c.stage](fc.Case(c.stage, c.name + "-plain", c.w, c.h, c.inp, dict(c.par, demod=0), scene=c.scene, nonfinite=c.nonfinite))


def _upsample_bound(L, glo, ghi, f, sigma):
    """The derived bound of the demodulated upsampling's hi layer and of vr_upsample.h's C before it, per word: -> (bound of L_p.rgb [H][W][3], D_e, D_s).
    The statement is a ratio of two sums over up to 16 taps, C = sum w_q c_q / sum w_q kappa_q with c_q = L_q.rgb / d_q, then L_p = (kappa_p C) d_p.
    Values: the tap's division, its product with the weight, at most 16 additions; the same for the denominator's product and additions; the quotient, the
    product with kappa_p, the product with d_p: 38 roundings of M = sum w_q |c_q| / D (times kappa_p d_p).
    Weights: a relative error delta_q of w_q moves C by at most delta_q w_q (|c_q| + |C|) / D -- it is in the numerator and in the denominator.  delta_q in
    roundings: the spline factor b(a) is at most 9 operations on intermediates of up to 13/6 against a result of 1/6 or more (b_1, b_2; b_0 and b_3 are
    products), 117, and a = r / 2f is one rounding that (1 - a)^3 amplifies by 3a / (1 - a) <= 15 at a = 5/6 (r / 4 and r / 8 are exact): 132 per axis, 265 for
    s = b_x b_y.  Where both coverages are positive e = w_n w_d w_a follows (two products, and one for s e): w_d = exp_(-x_d), x_d of 4 roundings, and
    w_a = exp_(-x_a), x_a of 7 (three differences, their squares, two sums, sigma^2, the quotient): an argument's relative error k comes out as k x, and exp_
    itself is good to 2; w_n = pow_(dot, sigma_n) = exp_(sigma_n log_(dot)): the dot product of two guides' normals is 5 roundings of magnitude 1 against dot,
    6 sigma_n / dot with the clamp, then 3 x_n for the logarithm's product and 2.  A dot below 6 x 2^-24 has no relative bound: there w_n is anywhere in
    [0, (12 x 2^-24)^sigma_n], an absolute error of the weight.  Every weight and every product of the sums may besides underflow: 2^-149 absolutely each."""
    L, glo, ghi = (np.asarray(a, np.float64) for a in (L, glo, ghi))
    sn, sd, sa = (float(np.float32(sigma[i])) for i in (1, 2, 4))
    h, w = L.shape[:2]
    H, W = f * h, f * w
    dlo, dhi = hd.spec_divisor(glo), hd.spec_divisor(ghi)
    c = L[..., :3] / dlo
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x0, y0 = np.floor_divide(2 * xs + 1 - f, 2 * f), np.floor_divide(2 * ys + 1 - f, 2 * f)
    bx = hu.spec_spline((2 * xs + 1 - f - 2 * f * x0) / (2.0 * f))
    by = hu.spec_spline((2 * ys + 1 - f - 2 * f * y0) / (2.0 * f))
    zero3 = np.zeros((H, W, 3))
    acc = {t: dict(N=zero3.copy(), M=zero3.copy(), D=np.zeros((H, W)), E=zero3.copy(), Ew=np.zeros((H, W)), A=zero3.copy()) for t in ("e", "s")}
    for j in range(4):
        for i in range(4):
            lx, ly = x0 - 1 + i, y0 - 1 + j
            ok = (lx >= 0) & (lx < w) & (ly >= 0) & (ly < h)
            cx, cy = np.clip(lx, 0, w - 1), np.clip(ly, 0, h - 1)
            gq, cq, kq = glo[cy, cx], c[cy, cx], L[cy, cx][..., 3]
            s = np.where(ok, bx[..., i] * by[..., j], 0.0)
            both = (ghi[..., 3] > 0) & (gq[..., 3] > 0)
            flat = ~ghi[..., 4:7].any(axis=-1) | ~gq[..., 4:7].any(axis=-1)
            dot = np.clip((ghi[..., 4:7] * gq[..., 4:7]).sum(axis=-1), 0.0, 1.0)
            loose = both & ~flat & (dot < 6 * U)
            with np.errstate(divide="ignore"):
                xn = np.where(flat | loose, 0.0, -sn * np.log(np.where(dot > 0, dot, 1.0)))
            xd = np.abs(ghi[..., 7] - gq[..., 7]) / (sd * np.maximum(ghi[..., 7], gq[..., 7]) + float(np.float32(1e-6)))
            da = ghi[..., 0:3] - gq[..., 0:3]
            xa = (da * da).sum(axis=-1) / (sa * sa)
            delta_e = 3 + np.where(flat | loose, 0.0, 6 * sn / np.where(dot > 0, dot, 1.0) + 3 * xn + 2) + (4 * xd + 2) + (7 * xa + 2)
            e = hu.spec_edge(ghi, gq, sigma)
            for t, wq, delta, absolute in (("e", s * e, 265 + np.where(both, delta_e, 0.0), np.where(loose, s * (12 * U) ** sn, 0.0) + TINY), ("s", s, 265.0, TINY)):
                a = acc[t]
                a["N"] += wq[..., None] * cq
                a["M"] += wq[..., None] * np.abs(cq)
                a["D"] += wq * kq
                a["E"] += ((delta * U * wq + absolute) * ok)[..., None] * np.abs(cq)      # the weight's error against the tap's value ...
                a["Ew"] += (delta * U * wq + absolute) * ok                                  # ... and against C
                a["A"] += TINY * ok[..., None]
    De, Ds = acc["e"]["D"], acc["s"]["D"]
    first, second = De > hu.MIN_WEIGHT, Ds > hu.MIN_WEIGHT
    bound = zero3.copy()
    for t, take in (("e", first), ("s", second & ~first)):
        a = acc[t]
        D = np.where(take, a["D"], 1.0)[..., None]
        C = np.abs(a["N"]) / D
        b = (38 * U * a["M"] + a["E"] + a["Ew"][..., None] * C + a["A"] * (1.0 + C)) / D
        bound = np.where(take[..., None], b, bound)
    k = ghi[..., 3]
    return bound * (k[..., None] * dhi) + TINY, De, Ds


@pytest.mark.parametrize("case_id", [c.id for c in fc.cases("demod")])
def test_demod(case_id):
    c = next(x for x in fc.cases("demod") if x.id == case_id)
    out = fc.host(c)
    poisoned = c.name.endswith("nan-inf-albedo")
    assert c.par["demod"] == 1 and (c.nonfinite or all(np.isfinite(a).all() for a in out.values())), c.id
    feats = [c.inp["glo"], c.inp["feat_hi"]] if c.stage == "upsample" else [c.inp["feat"]]
    census = _census(feats)
    assert min(census) >= 8, (c.id, census)                                      # every value of ALBEDOS on covered pixels
    # with demod 0 the catalogue runs the plain host function, on these inputs too
    plain = _plain_twin(c)
    with np.errstate(all="ignore"):
        if c.stage == "split":
            direct = {"S": hl.split(c.inp["y"], c.inp["B"], np.ascontiguousarray(c.inp["feat"][..., 3]))}
        elif c.stage == "merge":
            direct = dict(zip(("out", "L"), hl.merge(c.inp["F"], c.inp["B"], np.ascontiguousarray(c.inp["feat"][..., 3]))))
        elif c.stage == "prepare":
            direct = fc._prepare_host(fc.Case("prepare", "direct", c.w, c.h, c.inp, {"n": c.par["n"]}))
        else:
            f = c.par["f"]
            ghi = hu.guide(c.inp["feat_hi"])
            B, _ = hr.prepare(fc.oracle(c.scene, f * c.w, f * c.h), c.par["rays"], np.zeros((f * c.h, f * c.w, 4), np.float32))
            direct = dict(zip(("out", "L"), hu.upsample(c.inp["L"], c.inp["glo"], ghi, B, f, c.par["sigma"])))
    assert set(plain) == set(direct) == set(out) and all(_same_or_nan(plain[k], direct[k]) for k in plain), c.id
    # pixels without coverage hold albedo words and come out as the plain stage's, bit for bit
    fo = feats[-1]
    bare = (fo[..., 3] == 0) & (fo[..., 0:3] != 0).any(axis=-1)
    assert bare.sum() >= 8 and all(_same_or_nan(out[k][bare], plain[k][bare]) for k in out), (c.id, int(bare.sum()))
    if c.stage != "upsample" and c.par.get("n") != 1:
        assert any(not _same_or_nan(out[k], plain[k]) for k in out if k != "guide"), c.id
    _DEMOD_CHECKS[c.stage](c, out, plain, poisoned)


def _poison(c, twin_name):
    """a poisoned case: (the features before the poison's host outputs, NaN mask, inf mask, covered)"""
    twin = next(x for x in fc.cases("demod") if x.name == twin_name)
    feat = c.inp["feat"]
    is_nan, is_inf = np.isnan(feat[..., 0:3]), np.isposinf(feat[..., 0:3])
    covered = feat[..., 3] > 0
    assert np.isfinite(feat[..., 3:]).all() and not np.isneginf(feat).any()
    for m in (is_nan, is_inf):                                                   # on covered and on uncovered pixels, one channel of a pixel at most
        assert (m.sum(axis=-1) <= 1).all() and (m.any(axis=-1) & covered).sum() >= 8 and (m.any(axis=-1) & ~covered).sum() >= 4, c.id
    return twin, is_nan, is_inf, covered


def _demod_split(c, out, plain, poisoned):
    S, y, B, feat = out["S"], c.inp["y"], c.inp["B"], c.inp["feat"]
    kappa = feat[..., 3]
    assert _same(S[..., 3], kappa)
    if poisoned:
        twin, is_nan, is_inf, covered = _poison(c, "demod-albedos")
        clean = fc.host(twin)["S"][..., :3]
        hit = (is_nan | is_inf) & covered[..., None]
        assert np.isnan(S[..., :3][is_nan & covered[..., None]]).all() and not np.isnan(S[..., :3][~(is_nan & covered[..., None])]).any()      # that channel, and no other
        assert (S[..., :3][is_inf & covered[..., None]] == 0).all()              # an infinite albedo divides to 0
        assert _same(S[..., :3][~hit], clean[~hit])
        return
    with np.errstate(all="ignore"):
        want = hd.spec_split(y, B, feat)[..., :3]
        d = hd.spec_divisor(feat)
        bound = 4 * U * (np.abs(y[..., :3].astype(np.float64)) + np.abs((1.0 - kappa.astype(np.float64))[..., None] * B[..., :3])) / d + TINY
    fin = np.isfinite(S[..., :3])
    if c.nonfinite:                                                              # the quotient overflows: inf exactly where the float64 quotient leaves float32, by its sign
        over = np.abs(want) > FLT_MAX * (1 + 2 * U)
        assert not np.isnan(S).any() and over.sum() > 100 and fin.sum() > 100 and np.array_equal(~fin, over) and (np.sign(S[..., :3][over]) == np.sign(want[over])).all()
    else:
        assert fin.all()
    err = np.abs(S[..., :3] - want)
    assert _note("split", c, err[fin], bound[fin]) <= 1.0, c.id
    if c.name == "demod-subnormal-quotient":
        sub = (S[..., :3] != 0) & (np.abs(S[..., :3]) < SUBNORMAL)
        assert (sub & (feat[..., 0:3] == np.float32(1e5))).sum() >= 32 and (np.abs(y[..., :3]) >= SUBNORMAL * 0.8).all(), int(sub.sum())      # not flushed
    elif not c.nonfinite:
        assert (S[..., :3] < 0).mean() > 0.1 and (S[..., :3] > 0).mean() > 0.1   # signed


def _demod_prepare(c, out, plain, poisoned):
    v, g = out["v"], out["guide"]
    S, feat, counts, n = c.inp["S"], c.inp["feat"], c.inp.get("counts"), c.par["n"]
    n_px = np.full((c.h, c.w), n) if counts is None else ha.per_pixel(counts, c.w, c.h)
    assert _same_or_nan(g, plain["guide"])                                       # the guide stays prepare's
    with np.errstate(all="ignore"):
        scale = np.where(n_px >= 2, n_px / np.maximum(n_px - 1.0, 1.0), 0.0).astype(np.float32)
        var = np.where((n_px >= 2)[..., None], S * scale[..., None], np.float32(0.0))
        want = hd.spec_variance(var, feat, n_px)
        s2 = want * n_px                                                         # the statement squares before it divides: (s * s) / float(n)
    if poisoned:
        twin, is_nan, is_inf, covered = _poison(c, "demod-counts")
        nan_px = (is_nan & covered[..., None]).any(axis=-1)
        assert np.isnan(v[nan_px]).all() and np.isfinite(v[~nan_px]).all()       # NaN albedo, covered: a NaN v there and nowhere else (var = 0 too: 0 / NaN)
        clean = fc.host(twin)
        assert _same(v[~covered], plain["v"][~covered])
        untouched = ~((is_nan | is_inf).any(axis=-1) & covered)
        assert _same(v[untouched], clean["v"][untouched])
        words = np.ones(g.shape, bool)
        words[..., 0:3] = ~(is_nan | is_inf)
        assert _same(g[words], clean["guide"][words])                            # the guide copies the word, and no other word moves
        inf_px = (is_inf & covered[..., None]).any(axis=-1) & (n_px >= 2)        # an infinite albedo: that channel's share is 0
        assert np.abs(v[inf_px] - want[inf_px]).max() <= 2.0 ** -21 * want[inf_px].max() and (v[inf_px] < clean["v"][inf_px]).any()
        return
    assert (v[n_px < 2] == 0).all() and (n_px < 2).any() == (n == 1 or counts is not None)      # n = 1: var = 0 and v = 0
    fin = np.isfinite(v)
    if c.nonfinite:
        with np.errstate(all="ignore"):
            over = np.isinf(var[..., :3]).any(axis=-1) | (s2 > FLT_MAX * (1 - 2.0 ** -20))
            sure = np.isinf(var[..., :3]).any(axis=-1) | (s2 > FLT_MAX * (1 + 2.0 ** -20))
        assert not np.isnan(v).any() and np.isposinf(v[~fin]).all() and sure.sum() > 100 and fin.sum() > 100
        assert (~fin)[sure].all() and over[~fin].all()                           # inf where the variance or the square leaves float32, and nowhere else
    else:
        assert fin.all()
    with np.errstate(invalid="ignore"):
        err, bound = np.abs(v - want)[fin], (2.0 ** -21 * want + TINY)[fin]
    assert _note("prepare", c, err, bound) <= 1.0, c.id
    covered = feat[..., 3] > 0
    assert n == 1 or not _same(v[covered], plain["v"][covered])
    if c.name == "demod-tiny-n2":
        assert ((v > 0) & (v < SUBNORMAL)).sum() > 100, c.id
    if counts is not None:
        assert (counts == 1).any() and (n_px == 1).sum() > 100 and (v[(n_px >= 2) & covered] > 0).sum() > 100


def _demod_merge(c, out, plain, poisoned):
    o, L, F, B, feat = out["out"], out["L"], c.inp["F"], c.inp["B"], c.inp["feat"]
    kappa = feat[..., 3]
    assert _same(o[..., 3], kappa) and _same(L[..., 3], kappa)
    if poisoned:
        twin, is_nan, is_inf, covered = _poison(c, "demod-alpha-differs")
        clean = fc.host(twin)
        nan_w = is_nan & covered[..., None]
        hit = (is_nan | is_inf) & covered[..., None]
        for a, b in ((o, clean["out"]), (L, clean["L"])):
            assert np.isnan(a[..., :3][nan_w]).all() and not np.isnan(a[..., :3][~hit]).any() and _same(a[..., :3][~hit], b[..., :3][~hit])
        inf_w = is_inf & covered[..., None]
        assert not np.isfinite(L[..., :3][inf_w]).any()                          # F d: inf by F's sign, NaN where F is 0
        return
    with np.errstate(all="ignore"):
        so, sl = hd.spec_merge(F, B, feat)
        G = np.abs((1.0 - kappa.astype(np.float64))[..., None] * B[..., :3])
        bl = 3 * U * np.abs(sl[..., :3]) + TINY
        bo = 6 * U * (G + np.abs(sl[..., :3])) + TINY
    fl, fo = np.isfinite(L[..., :3]), np.isfinite(o[..., :3])
    if c.nonfinite:                                                              # the remodulation overflows
        over = np.abs(sl[..., :3]) > FLT_MAX * (1 + 4 * U)
        assert not np.isnan(L).any() and not np.isnan(o).any() and over.sum() > 100 and fl.sum() > 100
        assert (~fl)[over].all() and (np.abs(sl[..., :3])[~fl] > FLT_MAX * (1 - 4 * U)).all()
        assert (np.sign(L[..., :3][over]) == np.sign(sl[..., :3][over])).all() and (o[..., :3][over & (sl[..., :3] < 0)] == 0).all() and np.isposinf(o[..., :3][over & (sl[..., :3] > 0)]).all()
    else:
        assert fl.all() and fo.all()
    assert (o[..., :3] >= 0).all()
    assert _note("merge", c, np.abs(L[..., :3] - sl[..., :3])[fl], bl[fl]) <= 1.0 and _note("merge", c, np.abs(o[..., :3] - so[..., :3])[fo & fl], bo[fo & fl]) <= 1.0, c.id
    if c.name == "demod-alpha-is-kappa":
        assert _same(F[..., 3], kappa)
    elif c.name == "demod-alpha-differs":
        assert ((F[..., 3] <= hl.MIN_WEIGHT) & (kappa > 0)).sum() > 100 and ((F[..., 3] > hl.MIN_WEIGHT) & (F[..., 3] != kappa)).sum() > 100


def _demod_upsample(c, out, plain, poisoned):
    f = c.par["f"]
    L, glo = c.inp["L"], c.inp["glo"]
    ghi = hu.guide(c.inp["feat_hi"])
    B, _ = hr.prepare(fc.oracle(c.scene, f * c.w, f * c.h), c.par["rays"], np.zeros((f * c.h, f * c.w, 4), np.float32))
    o, Lh = out["out"], out["L"]
    assert np.isfinite(c.inp["feat_hi"]).all() and np.isfinite(glo).all() and np.isfinite(L).all()      # no non-finite word goes into this stage
    assert (o[..., :3] >= 0).all() and _same(o[..., 3], ghi[..., 3]) and _same(Lh[..., 3], ghi[..., 3])
    so2, sl2 = hd.upsample(L, glo, ghi, B, f, c.par["sigma"], staged=True)       # the kernel's window holds the same values
    assert _same(o, so2) and _same(Lh, sl2)
    rep = np.repeat(np.repeat(glo, f, axis=0), f, axis=1)
    equal = (ghi.view(np.uint32) == rep.view(np.uint32)).all(axis=-1) & (ghi[..., 3] > 0)
    assert equal.sum() >= 5, (c.id, int(equal.sum()))                            # the existing checkerboard: a hi guide equal to the lo tap's under it
    none = ghi[..., 3] == 0
    assert _same(o[none][:, :3], B[none][:, :3]) and not Lh[none].any()
    so, sl = hd.spec_upsample(L, glo, ghi, B, f, c.par["sigma"])
    bound, De, Ds = _upsample_bound(L, glo, ghi, f, c.par["sigma"])
    near = (np.abs(De - hu.MIN_WEIGHT) < 1e-3 * hu.MIN_WEIGHT) | (np.abs(Ds - hu.MIN_WEIGHT) < 1e-3 * hu.MIN_WEIGHT)
    assert near.mean() <= 0.01, (c.id, float(near.mean()))                       # the float64 statement alone stays inside the cap
    k = ghi[..., 3].astype(np.float64)
    G = np.abs((1.0 - k)[..., None] * B[..., :3])
    bo = bound + 3 * U * (G + np.abs(sl[..., :3])) + TINY                        # G's two roundings and the sum's
    assert _note("upsample", c, np.abs(Lh[..., :3] - sl[..., :3])[~near], bound[~near]) <= 1.0 and _note("upsample", c, np.abs(o[..., :3] - so[..., :3])[~near], bo[~near]) <= 1.0, c.id
    covered = ghi[..., 3] > 0
    assert not _same(Lh[covered], plain["L"][covered])
    assert ((De > hu.MIN_WEIGHT) & covered).any() and ((De <= hu.MIN_WEIGHT) & (Ds > hu.MIN_WEIGHT) & covered).any()      # both tiers


_DEMOD_CHECKS = {"split": _demod_split, "prepare": _demod_prepare, "merge": _demod_merge, "upsample": _demod_upsample}


def test_demod_worst_errors_are_printed():
    """per stage, the worst host-against-float64 error of the finite words of the group as a share of its derived bound (collected by test_demod above)"""
    if not _WORST:
        for c in fc.cases("demod"):
            test_demod(c.id)
    for stage in ("split", "prepare", "merge", "upsample"):
        print("demod %-8s worst error / derived bound %.3f (%s)" % ((stage,) + _WORST[stage]))
        assert _WORST[stage][0] <= 1.0


# ---- adaptive error ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("adaptive_error"))
def test_adaptive_error(name):
    c = next(x for x in fc.cases("adaptive_error") if x.name == name)
    e = fc.host(c)["e"]
    tiles, counts = c.inp["tiles"], c.inp["counts"]
    ty, tx = ha.tiles_of(c.w, c.h)
    full = np.full(ty * tx, 2, np.int32)
    full[tiles] = counts
    with np.errstate(all="ignore"):
        want = ha.spec_tile_error(c.inp["fb"], c.inp["S"], full.reshape(ty, tx)).reshape(-1)[tiles]
    assert np.isposinf(e[counts == 1]).all()
    assert {2, 8} <= set(tiles.tolist())                 # the ragged corner tiles
    if c.nonfinite:
        assert np.isnan(e[tiles == 4]).all() and np.isfinite(e[tiles != 4]).all() and np.array_equal(np.isnan(e), np.isnan(want))
        return
    _close_adaptive(e, want)
    if name == "all-tiles":
        assert {1, 2, 1000} <= set(counts.tolist()) and not c.inp["fb"][16:32, 16:32, :3].any()
        at = int(np.nonzero(tiles == 4)[0][0])           # the black tile: its error is relative to the floor alone
        assert np.isfinite(e[at]) and e[at] > 0
