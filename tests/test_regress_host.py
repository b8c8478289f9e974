"""CPU: the one-pass local-regression filter (volren_amd/csrc/vr_regress.h) built for the host (tests/hostkernel/regress_host.cpp): against a float64 numpy
statement of the header (tests/hk_regress.py) on oracle frames; its identities on synthetic frames; what it does to the error of oracle frames next to the
layered a-trous at its defaults; the sweep of "denoise_ridge" that chose the default; and a temporal sequence.  tests/test_gpu_regress.py holds the HIP kernel to
this build bit for bit.  The frames, guides and references are tests/test_resolve_host.py's own, traced once per process."""
import numpy as np
import pytest

import hk_layers as hl
import hk_regress as hg
import hk_resolve as hr
import scenes
import test_resolve_host as trh
from hk_common import same as _same
from test_layers_host import _resolved

W, H, RAYS = trh.W, trh.H, trh.RAYS
SCENES = trh.SCENES
RIDGE = hg.default_ridge()
RIDGES = (0.0, 1.0)                              # zero order, and a first-order fit: every identity below holds for both


def test_the_constants_are_the_headers():
    assert hg.constants()[:7] == (hg.RADIUS, hg.TERMS, hg.MIN_WEIGHT, hg.MIN_DEPTH, hg.PIVOT_FLOOR, hg.RIDGE_MIN, hg.RIDGE_MAX)
    assert RIDGE in SWEEP
    for v, ok in ((0.0, True), (2.0 ** -20, True), (2.0 ** 20, True), (1.0, True), (2.0 ** -21, False), (2.0 ** 20 * 1.5, False), (-1.0, False), (float("nan"), False),
                  (float("inf"), False)):
        assert hg.ridge_ok(v) == ok, v


# ---- 1: the host build is the header ------------------------------------------------------------------------------------------------------------------
# largest |host - float64 statement| of F.rgb per channel over both frame sizes, recorded from the host build; asserted at 4x
# (tests/test_filter_cases_host.py holds crafted frames of larger values to these too, times magnitude / the magnitude measured here: its _scaled)
# (ridge 0, ridge 1)
RECORDED = {"c2": ((1.96e-7, 2.14e-7, 1.71e-7), (2.58e-7, 2.55e-7, 1.76e-7)),
            "c3env": ((2.56e-8, 2.21e-8, 3.32e-8), (2.60e-8, 2.57e-8, 4.31e-8)),
            "c4_64": ((5.49e-7, 4.67e-7, 3.94e-7), (5.66e-7, 4.40e-7, 3.85e-7))}


@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_matches_the_float64_statement(name):
    """Frames of 8 spp at 64x48 and 48x32 against 2 x 2 expected rays, with "denoise_ridge" 0 and 1: F against hk_regress.spec of the host's S and
    guide.  F.a is kappa bit for bit."""
    worst = np.zeros((2, 3))
    for w, h in ((64, 48), (48, 32)):
        y, B, _, feat = _resolved(name, 8, w, h, most=64 if (w, h) == (W, H) else 8)
        kappa = feat[..., 3]
        for i, ridge in enumerate(RIDGES):
            out, L, S, F = hg.layered(y, B, feat, ridge)
            assert np.isfinite(out).all() and (out[..., :3] >= 0).all()
            assert _same(F[..., 3], kappa) and _same(L[..., 3], kappa) and _same(out[..., 3], kappa)
            big = kappa > hl.MIN_WEIGHT
            assert _same(L[..., :3][big], (F[..., :3] * np.float32(1))[big])                # the merge's ratio is kappa / kappa = 1
            want = hg.spec(S, hg._guide(feat), ridge)
            worst[i] = np.maximum(worst[i], np.abs(F - want)[..., :3].max(axis=(0, 1)))
        assert not _same(hg.layered(y, B, feat, 0.0)[3], hg.layered(y, B, feat, 1.0)[3])
    print("%s: ridge 0 %s   ridge 1 %s" % (name, " ".join("%.3g" % x for x in worst[0]), " ".join("%.3g" % x for x in worst[1])))
    assert (worst <= 4 * np.array(RECORDED[name])).all()


def test_the_solve_against_numpy_on_random_systems():
    """regress_solve on 200 random ridged systems of the filter's shape (A = sum w x x^T over 40 taps, x_0 = 1, plus lambda A_00 on the seven slopes, lambda
    = 0.01): beta_0 against numpy's float64 solve of the same float32 system.  The system is congruent to diag(A_00, A_00 (Cov + lambda I)) by a shear of norm at most
    1 + |xbar|^2 <= 8, so its condition number is below 8 * 8 * (8 + lambda) / lambda < 2^16 at the very worst; 40 random taps keep Cov near I / 3 and the
    number near 2^5, and float32 elimination then loses about 5 of its 24 bits.  Asserted at 2^-12 of the targets' range, 2."""
    rs = np.random.RandomState(11)
    for _ in range(200):
        x = np.concatenate([np.ones((40, 1)), rs.uniform(-1.0, 1.0, (40, 7))], axis=1)
        w = rs.uniform(0.0, 1.0, 40)
        c = rs.uniform(-2.0, 2.0, (40, 3))
        A = (w[:, None, None] * x[:, :, None] * x[:, None, :]).sum(axis=0)
        b = (w[:, None, None] * x[:, :, None] * c[:, None, :]).sum(axis=0)
        A = A + 0.01 * A[0, 0] * np.diag([0.0] + [1.0] * 7)
        A32, b32 = A.astype(np.float32), b.astype(np.float32)
        got = hg.solve(np.triu(A32), b32, 2.0 ** -20 * 0.01 * A[0, 0])
        want = np.linalg.solve(A32.astype(np.float64), b32.astype(np.float64))[0]
        assert np.abs(got - want).max() <= 2.0 ** -12 * 2.0


def test_an_emptied_column_is_dropped_and_the_rest_is_fitted_without_it():
    """a system whose column 3 is all zeros but for a pivot at the floor itself (not above it), and the same with a NaN pivot: beta_0 is that of the system without
    row and column 3 -- here the 2 x 2 system of the intercept and column 1"""
    A = np.zeros((8, 8), np.float32)
    b = np.zeros((8, 3), np.float32)
    A[0, 0], A[0, 1], A[1, 1] = 4.0, 2.0, 3.0
    for i in range(2, 8):
        A[i, i] = 1.0
    b[0], b[1] = (8.0, 4.0, -2.0), (5.0, 1.0, 0.5)
    want = np.linalg.solve(np.array([[4.0, 2.0], [2.0, 3.0]]), b[:2].astype(np.float64))[0]
    for pivot in (0.25, float("nan")):
        A[3, 3] = pivot
        b[3] = (7.0, 7.0, 7.0)                         # a right-hand side the dropped column must not spread
        got = hg.solve(A, b, 0.25)
        assert np.abs(got - want).max() <= 2.0 ** -20, (pivot, got, want)
    A[3, 3] = 0.5                                      # above the floor: kept, and being decoupled it changes nothing either
    assert np.abs(hg.solve(A, b, 0.25) - want).max() <= 2.0 ** -20


# ---- 2: identities ---------------------------------------------------------------------------------------------------------------------------------------
def test_pixels_without_coverage_give_the_background_bit_for_bit():
    """on oracle frames (the sky around c3env's and c2's volumes), whatever the ridge, and on a frame with no coverage anywhere"""
    for name in ("c3env", "c2"):
        y, B, _, feat = _resolved(name, 8)
        none = feat[..., 3] == 0
        assert none.sum() > 500
        for ridge in RIDGES:
            out, L, S, F = hg.layered(y, B, feat, ridge)
            assert _same(out[none][:, :3], B[none][:, :3]) and not np.abs(L[none]).any() and not np.abs(F[none]).any()
            assert np.abs(S[none][:, :3]).max() > 1e-3 and not _same(y[none][:, :3], B[none][:, :3])      # (the frame's sky is sampled, B's is the quadrature)
    rs = np.random.RandomState(4)
    y = rs.uniform(0.0, 2.0, (20, 30, 4)).astype(np.float32)
    B = np.zeros((20, 30, 4), np.float32)
    B[..., :3] = rs.uniform(0.0, 3.0, (20, 30, 3))
    feat = rs.uniform(0.1, 1.0, (20, 30, 8)).astype(np.float32)
    feat[..., 3] = 0.0
    out, L, _, F = hg.layered(y, B, feat, 1.0)
    assert _same(out[..., :3], B[..., :3]) and not out[..., 3].any() and not L.any() and not F.any()


def _flat_guide(h, w, depth):
    """a guide whose edge factors are 1 under sigma_d = 2^60: full coverage, one albedo, no normal"""
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3] = 0.5
    g[..., 3] = 1.0
    g[..., 7] = depth
    return g


FLAT_SIGMA = (4.0, 0.5, 2.0 ** 60, 0.25, 0.2)


def test_a_layer_affine_in_depth_comes_back_as_itself_and_zero_order_does_not_give_it():
    """The test that says the regression is a regression.  kappa = 1, depth d a curved function of the position (so no symmetry of the window stands in for the
    fit), C = c0 + c1 d exactly, every tap's edge factor 1 (sigma_d = 2^60: exp(-|dd| / (2^60 d + 1e-6)) = 1 in float32), lambda = 2^-20.  Per pixel, with xbar,
    m2 and v = m2 - xbar^2 the weighted mean, second moment and variance of the depth regressor x = (d_q - d_p) / d_p in its window (float64, from the frame):
      zero order returns the window's weighted mean of C, which misses C_p by |c1| d_p |xbar| exactly;
      the ridged fit of an exactly affine target has slope b1 v / (v + lambda), b1 = c1 d_p, and misses C_p by lambda |b1 xbar| / (v + lambda);
      float32: a sum of n = 121 terms carries a relative n u at most, u = 2^-24.  The slope is a quotient of two differences, (B_1 - A_01 B_0 / A_00) over
      (A_11 - A_01^2 / A_00 + ridge): each is off by at most 4 n u times its larger term, A_00 sqrt(m2) |C|max and A_00 m2, while their exact values are
      A_00 b1 v and A_00 v -- so the slope is off by 4 n u (|b1| m2 + sqrt(m2) |C|max) / v, the intercept by |xbar| times that plus 2 n u |C|max for B_0 / A_00.
    Asserted: first order within the sum of the two bounds at every pixel; zero order at its analytic miss to 2 n u |C|max, above 0.1 somewhere, and beyond the
    first-order bound on more than half of the frame."""
    h, w = 24, 40
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    depth = (2.0 + 0.004 * (xx - 8.0) ** 2 + 0.003 * xx * yy + 0.05 * yy).astype(np.float32)
    guide = _flat_guide(h, w, depth)
    d64 = depth.astype(np.float64)
    c0, c1 = np.array([0.3, 1.0, -0.5]), np.array([0.2, -0.1, 0.3])
    C = c0 + c1 * d64[..., None]
    cmax = 3.0
    assert np.abs(C).max() <= cmax
    S = np.concatenate([C, np.ones((h, w, 1))], axis=2).astype(np.float32)
    lam = 2.0 ** -20
    A, _ = hg.spec_sums(S, guide, FLAT_SIGMA)
    xbar = A[..., 0, 1] / A[..., 0, 0]
    m2 = A[..., 1, 1] / A[..., 0, 0]
    v = m2 - xbar * xbar
    b1 = np.abs(c1).max() * d64
    nu = 121 * 2.0 ** -24
    bias = lam * b1 * np.abs(xbar) / (v + lam)
    rounding = np.abs(xbar) * 4 * nu * (b1 * m2 + np.sqrt(m2) * cmax) / v + 2 * nu * cmax
    miss0 = np.abs(c1)[None, None, :] * (d64 * np.abs(xbar))[..., None]
    first = hg.regress(S, guide, lam, FLAT_SIGMA)
    zero = hg.regress(S, guide, 0.0, FLAT_SIGMA)
    err1 = np.abs(first[..., :3] - C).max(axis=-1)
    err0 = np.abs(zero[..., :3] - C)
    print("affine in depth: first order misses by %.3g at most (bounds: ridge %.3g, rounding %.3g), zero order by %.3g (median %.3g)"
          % (err1.max(), bias.max(), rounding.max(), err0.max(), np.median(err0.max(axis=-1))))
    assert (err1 <= bias + rounding).all()
    assert np.abs(err0 - miss0).max() <= 2 * nu * cmax + 2.0 ** -22
    assert miss0.max() > 0.1 and (err0.max(axis=-1) > bias + rounding).mean() > 0.5


def test_one_nan_texel_poisons_the_pixels_whose_window_holds_it_and_no_other():
    y, B, _, feat = _resolved("c4_64", 8)
    kappa = feat[..., 3]
    S = hl.split(y, B, kappa)
    guide = hg._guide(feat)
    py, px = 20, 30
    assert kappa[py, px] > 0.5
    S[py, px, 1] = np.nan
    yy, xx = np.mgrid[0:H, 0:W]
    near = (np.abs(yy - py) <= hg.RADIUS) & (np.abs(xx - px) <= hg.RADIUS)
    for ridge in RIDGES:
        F = hg.regress(S, guide, ridge)
        bad = ~np.isfinite(F).all(axis=-1)
        assert not bad[~near].any()
        assert np.array_equal(bad, near & (kappa != 0)), ridge          # dense grid: every tap's edge factor is positive, so every such window counts the texel
    S[py, px, 1] = 0.0
    g = guide.copy()
    g[py, px, 7] = np.nan                                                # the same for the guide's depth
    bad = ~np.isfinite(hg.regress(S, g, 1.0)).all(axis=-1)
    assert bad[py, px] and not bad[~near].any()


@pytest.mark.parametrize("w,h", ((1, 37), (37, 1), (5, 5)))
def test_frames_smaller_than_the_window(w, h):
    rs = np.random.RandomState(w + h)
    S = rs.uniform(-1.0, 2.0, (h, w, 4)).astype(np.float32)
    kappa = rs.uniform(0.05, 1.0, (h, w)).astype(np.float32)
    kappa[0, 0] = 0.0
    S[..., 3] = kappa
    S[..., :3] *= kappa[..., None]
    guide = _flat_guide(h, w, rs.uniform(1.0, 3.0, (h, w)).astype(np.float32))
    guide[..., 3] = kappa
    guide[..., 0:3] = rs.uniform(0.2, 0.8, (h, w, 3))
    for ridge in RIDGES:
        F = hg.regress(S, guide, ridge)
        want = hg.spec(S, guide, ridge)
        assert np.isfinite(F).all() and not F[0, 0].any() and _same(F[..., 3], kappa)
        assert np.abs(F - want).max() <= 2.0 ** -16                     # sums of at most 37 terms of values below 2, solved under a ridge of 1
    o = trh._oracle("c2", w, h)
    import hk_expected as he
    feat = he.expected_pass(o, RAYS)
    yo, Bo = hr.resolved(o, RAYS, o.render(4), feat)
    assert np.isfinite(hg.layered(yo, Bo, feat, 1.0)[0]).all()


# ---- 3: what it does to the error --------------------------------------------------------------------------------------------------------------------
SPPS = (2, 4, 16, 64)
TABLE_SCENES = ("c2", "c3", "c3env", "c4_64", "c2hid")
STRICT = {("c2", 4), ("c2", 16), ("c3", 4), ("c3", 16), ("c4_64", 4), ("c4_64", 16)}      # regression <= 1.0 x layered; every other cell <= 1.05 x
SWEEP = (0.0, 0.01, 0.1, 1.0, 10.0)
_CELLS = {}


def _cells(name, spp):
    """(layered a-trous at its defaults, the regression at each ridge of SWEEP) on the frame of `spp` samples: relative L2 of RGB against 1024 spp"""
    if (name, spp) not in _CELLS:
        y, B, var, feat = _resolved(name, spp)
        ref = trh._reference(name)
        _CELLS[name, spp] = (scenes.rel_l2(hl.layered(y, B, var, feat, spp)[0][..., :3], ref),
                             tuple(scenes.rel_l2(hg.layered(y, B, feat, ridge)[0][..., :3], ref) for ridge in SWEEP))
    return _CELLS[name, spp]


@pytest.mark.parametrize("name", TABLE_SCENES)
def test_the_error_next_to_the_layered_atrous(name):
    """Oracle frames at 64x48 of seed 42 (samples 1..n of one run), 2 x 2 expected rays, default sigmas; relative L2 of RGB over the whole frame against 1024 spp
    of seed 1234567.  c3env = c3 with show_environment 1, c2hid = c2 with show_environment 0.  Measured with the product's float32 code (layered a-trous at its
    defaults -> the regression at the default ridge):
                 2 spp              4 spp              16 spp             64 spp
      c2         0.0765 -> 0.0511   0.0555 -> 0.0421   0.0314 -> 0.0271   0.0257 -> 0.0236
      c3         0.6167 -> 0.4026   0.3919 -> 0.2645   0.2585 -> 0.2260   0.1981 -> 0.2001
      c3env      0.0207 -> 0.0147   0.0156 -> 0.0132   0.0122 -> 0.0113   0.0106 -> 0.0106
      c4_64      0.0978 -> 0.0533   0.0755 -> 0.0451   0.0514 -> 0.0362   0.0360 -> 0.0300
      c2hid      0.2221 -> 0.1562   0.1656 -> 0.1288   0.0951 -> 0.0825   0.0784 -> 0.0729
    It wins 18 of the 20 cells, by up to 46 %; c3 at 64 spp loses 1.0 % and c3env at 64 spp 0.2 %.
    Asserted: regression <= 1.0 x layered at 4 and 16 spp on c2, c3 and c4_64, <= 1.05 x in every other cell."""
    cells = {spp: _cells(name, spp) for spp in SPPS}
    at = SWEEP.index(RIDGE)
    print("%-6s %s" % (name, "   ".join("%3d spp %.4f -> %.4f" % (spp, cells[spp][0], cells[spp][1][at]) for spp in SPPS)))
    for spp in SPPS:
        base, reg = cells[spp][0], cells[spp][1][at]
        assert np.isfinite(base) and np.isfinite(reg)
        assert reg <= (1.0 if (name, spp) in STRICT else 1.05) * base, (name, spp, base, reg)


def test_the_sweep_of_the_ridge_decides_the_default():
    """The regression's error over the layered a-trous's, per cell of the table above, at "denoise_ridge" 0 (zero order), 0.01, 0.1, 1 and 10; the geometric mean
    of the 20 ratios per value:
                        0      0.01    0.1     1       10
      c2      2 spp    0.669   1.280   0.970   0.717   0.674
      c2      4 spp    0.759   1.321   1.008   0.794   0.762
      c2     16 spp    0.864   1.119   0.951   0.872   0.865
      c2     64 spp    0.921   1.007   0.956   0.926   0.922
      c3      2 spp    0.653   1.257   0.951   0.705   0.658
      c3      4 spp    0.675   1.165   0.889   0.708   0.678
      c3     16 spp    0.875   0.946   0.888   0.872   0.874
      c3     64 spp    1.010   0.931   0.972   1.000   1.009
      c3env   2 spp    0.708   1.208   0.940   0.746   0.712
      c3env   4 spp    0.846   1.240   1.002   0.867   0.848
      c3env  16 spp    0.930   1.024   0.959   0.932   0.930
      c3env  64 spp    1.002   0.948   0.979   0.997   1.002
      c4_64   2 spp    0.544   0.599   0.549   0.544   0.544
      c4_64   4 spp    0.597   0.596   0.585   0.595   0.597
      c4_64  16 spp    0.704   0.625   0.667   0.699   0.704
      c4_64  64 spp    0.833   0.699   0.778   0.825   0.832
      c2hid   2 spp    0.703   1.333   0.999   0.747   0.708
      c2hid   4 spp    0.778   1.335   1.016   0.807   0.780
      c2hid  16 spp    0.867   1.118   0.946   0.872   0.868
      c2hid  64 spp    0.930   1.020   0.965   0.934   0.930
      geometric mean   0.782   1.006   0.886   0.798   0.784
    The slopes pay where the guide explains a gradient of C and the window holds enough samples -- the dense c4_64 from 16 spp on gains a further 11-16 % at 0.01,
    c3 and c3env at 64 spp 5-8 % -- and cost on thin smoke at 2 and 4 spp, where 0.01 ends 17-34 % behind the a-trous that zero order beats by 15-35 %; a larger ridge trades both away and tends to zero order (10 is
    within 1 % of 0 everywhere).  The rule, fixed before the sweep was read: the default is the value with the smallest geometric mean.  That is 0."""
    ratios = np.array([[np.array(_cells(name, spp)[1]) / _cells(name, spp)[0] for spp in SPPS] for name in TABLE_SCENES])      # [scene][spp][ridge]
    for i, name in enumerate(TABLE_SCENES):
        for j, spp in enumerate(SPPS):
            print("%-6s %3d spp  %s" % (name, spp, "  ".join("%.3f" % r for r in ratios[i, j])))
    mean = np.exp(np.log(ratios).mean(axis=(0, 1)))
    print("ridge      %s" % "  ".join("%5g" % r for r in SWEEP))
    print("geo. mean  %s" % "  ".join("%.3f" % m for m in mean))
    assert SWEEP[int(np.argmin(mean))] == RIDGE


# ---- 4: temporal -----------------------------------------------------------------------------------------------------------------------------------------
def test_eight_frames_of_2_spp_under_a_fixed_camera_are_recorded():
    """c3env, frame k = samples 2k + 1, 2k + 2 of the run of seed 42, alpha 0.2: the last frame's error, 0.0122 -> 0.0113 (measured, layered a-trous -> the
    regression at the default ridge).
    Nothing is asserted but that both are finite."""
    from test_gpu_features import _replay
    from test_layers_host import ALPHA, _camera
    trh._inputs("c3env", 2)
    L = trh._RADIANCE["c3env", W, H, 64]
    o, feat = trh._oracle("c3env"), trh._guide("c3env")
    a, b = hl.Replay(), hg.Replay()
    for k in range(8):
        mu, S = _replay(L[2 * k:2 * k + 2])
        y, B = hr.resolved(o, RAYS, mu, feat)
        var = (S * np.float32(2)).astype(np.float32)
        ea = a.frame(_camera(o), y, B, var, feat, 2, ALPHA)[3]
        eb = b.frame(_camera(o), y, B, var, feat, 2, ALPHA, RIDGE)[3]
    ref = trh._reference("c3env")
    ea, eb = scenes.rel_l2(ea[..., :3], ref), scenes.rel_l2(eb[..., :3], ref)
    print("c3env, 8 frames of 2 spp, fixed camera: %.4f -> %.4f" % (ea, eb))
    assert np.isfinite(ea) and np.isfinite(eb)
