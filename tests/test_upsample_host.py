"""CPU: the upsampling of the scattered layer (volren_amd/csrc/vr_upsample.h) built for the host (tests/hostkernel/upsample_host.cpp): against a float64 numpy
statement of the header (tests/hk_upsample.py) on oracle frames; its identities on synthetic frames; the index arithmetic of the window its kernel stages
(vr_tiles.h ScaledTileWindow); and what it does to the error of oracle frames next to today's best call at equal samples.  tests/test_gpu_upsample.py holds
the HIP kernel to this build bit for bit.  The lo frames, guides and radiances are tests/test_resolve_host.py's own, traced once per process."""
import numpy as np
import pytest

import hk_layers as hl
import hk_resolve as hr
import hk_temporal as ht
import hk_upsample as hu
import scenes
import test_resolve_host as trh
from hk_common import same as _same

RAYS = trh.RAYS
SCENES = ("c2", "c3env", "c3", "c4_64")          # smoke.brick in front of the sky; under the LUT with the sky shown; under the LUT as configured (sky hidden); dense fp16
SIGMA = hu.hk_denoise.DEFAULT_SIGMA
U = 2.0 ** -24                                   # the unit roundoff of float32


def _lo_layer(name, spp, w, h, most):
    """(L, lo guide) of the layered filter on the oracle frame of seed 42 at w x h"""
    fb, var = trh._inputs(name, spp, w, h, most)
    feat = trh._guide(name, w, h)
    y, B = hr.resolved(trh._oracle(name, w, h), RAYS, fb, feat)
    return hl.layered(y, B, var, feat, spp)[1], hu.guide(feat)


_HI = {}


def _hi(name, W, H):
    """(hi guide, B) at W x H, marched once per process"""
    if (name, W, H) not in _HI:
        feat, B = hu.hi_inputs(trh._oracle(name, W, H), RAYS)
        _HI[name, W, H] = (hu.guide(feat), B)
    return _HI[name, W, H]


# ---- 1: the host build is the header ------------------------------------------------------------------------------------------------------------------
# largest |host - float64 statement| per channel over f = 2 and 3, recorded from the host build; asserted at 4x
# (out, L)
RECORDED = {"c2": ((1.19e-7, 1.15e-7, 7.99e-8), (1.24e-7, 1.09e-7, 7.64e-8)),
            "c3env": ((6.96e-8, 6.54e-8, 5.92e-8), (1.82e-8, 1.47e-8, 2.61e-8)),
            "c3": ((1.43e-8, 1.37e-8, 2.06e-8), (1.43e-8, 1.37e-8, 2.06e-8)),
            "c4_64": ((2.47e-7, 2.31e-7, 1.49e-7), (2.40e-7, 2.15e-7, 1.42e-7))}


@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_matches_the_float64_statement(name):
    """The layer of an 8-spp frame at 32x24 under hi guides of 64x48 (f = 2) and 96x72 (f = 3), 2 x 2 expected rays: out and L against hk_upsample.spec_upsample
    fed with the same float32 layer, guides and B.  Each is 16 products and sums of values below 4, one division and two or three more roundings; the alphas are
    kappa_p bit for bit.  A pixel whose float64 D_e or D_s lies within 1e-3 relative of 2^-20 may take the other tier in float32 and is left out: at most 0.1 %."""
    w, h = 32, 24
    L, glo = _lo_layer(name, 8, w, h, 8)
    worst = np.zeros((2, 3))
    for f in (2, 3):
        ghi, B = _hi(name, f * w, f * h)
        out, Lh = hu.upsample(L, glo, ghi, B, f)
        want_out, want_l, De, Ds = hu.spec_upsample(L, glo, ghi, B, f)
        assert np.isfinite(out).all() and np.isfinite(Lh).all() and (out[..., :3] >= 0).all()
        assert _same(out[..., 3], ghi[..., 3]) and _same(Lh[..., 3], ghi[..., 3])
        near = (np.abs(De - hu.MIN_WEIGHT) < 1e-3 * hu.MIN_WEIGHT) | (np.abs(Ds - hu.MIN_WEIGHT) < 1e-3 * hu.MIN_WEIGHT)
        assert near.mean() <= 1e-3, (f, int(near.sum()))
        for i, (got, want) in enumerate(((out, want_out), (Lh, want_l))):
            worst[i] = np.maximum(worst[i], np.abs(got - want)[~near][:, :3].max(axis=0))
        assert (De > hu.MIN_WEIGHT).sum() > 500                             # the edge tier carries the covered pixels
    print("%s: out %s   L %s" % ((name,) + tuple(" ".join("%.3g" % x for x in row) for row in worst)))
    assert (worst <= 4 * np.array(RECORDED[name])).all()


# ---- 2: identities ---------------------------------------------------------------------------------------------------------------------------------------
COLOUR = np.array([0.3, 0.7, 0.45])


def _flat_guide(kappa, depth=2.0):
    """a guide whose edge factor is 1 between any two pixels: one albedo, no normal, one depth"""
    h, w = kappa.shape
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3] = 0.5
    g[..., 3] = kappa
    g[..., 7] = depth
    return g


def _synthetic(w, h, f, seed=11):
    """kappa_q, kappa_p random in (0, 1] with some zeros among kappa_p, B random in [0, 3], L_q = kappa_q COLOUR"""
    rs = np.random.RandomState(seed)
    kq = rs.uniform(0.05, 1.0, (h, w)).astype(np.float32)
    kp = rs.uniform(0.05, 1.0, (f * h, f * w)).astype(np.float32)
    kp[rs.uniform(size=kp.shape) < 0.2] = 0.0
    B = np.zeros((f * h, f * w, 4), np.float32)
    B[..., :3] = rs.uniform(0.0, 3.0, (f * h, f * w, 3))
    L = np.concatenate([kq.astype(np.float64)[..., None] * COLOUR, kq[..., None]], axis=2).astype(np.float32)
    return L, kq, kp, B


def _is_the_constant(Lh, kp):
    """L_p.rgb = kappa_p C with C = COLOUR to the rounding of L_q (1), the 16 products (1 each side), the two sums of 16 positive terms (15 each), the division
    (1) and kappa_p C (1): 35 U relative, no cancellation anywhere"""
    want = kp.astype(np.float64)[..., None] * COLOUR
    assert (np.abs(Lh[..., :3] - want) <= 35 * U * want).all()
    assert _same(Lh[..., 3], kp)


@pytest.mark.parametrize("f", (2, 3, 4))
def test_a_constant_colour_comes_back_under_a_flat_guide_and_pixels_without_coverage_are_the_background(f):
    L, kq, kp, B = _synthetic(13, 9, f)
    out, Lh = hu.upsample(L, _flat_guide(kq), _flat_guide(kp), B, f)
    _is_the_constant(Lh, kp)
    assert _same(out[..., 3], kp)
    none = kp == 0
    assert none.sum() > 20 and _same(out[none][:, :3], B[none][:, :3]) and not np.abs(Lh[none]).any()
    want = np.maximum(0.0, (1.0 - kp.astype(np.float64))[..., None] * B[..., :3] + kp.astype(np.float64)[..., None] * COLOUR)
    assert np.abs(out[..., :3] - want).max() <= 2.0 ** -21               # G, L and their sum: three roundings of values below 4


def test_a_depth_edge_leaves_some_pixels_the_spatial_tier_alone():
    """the hi guide sees a band at depth 2000 that no lo pixel has: with sigma_d = 2^-8 every tap's w_d is exp(-255) -- 0 in float32 -- there, D_e = 0 and the plain spline
    answers; beside the band the edge tier does.  Both give the constant."""
    f = 2
    L, kq, kp, B = _synthetic(13, 9, f)
    ghi = _flat_guide(kp)
    ghi[:, 10:14, 7] = 2000.0
    sigma = (SIGMA[0], SIGMA[1], 2.0 ** -8, SIGMA[3], SIGMA[4])
    out, Lh = hu.upsample(L, _flat_guide(kq), ghi, B, f, sigma)
    _, _, De, Ds = hu.spec_upsample(L, _flat_guide(kq), ghi, B, f, sigma)
    band = (ghi[..., 7] == 2000.0) & (kp > 0)
    assert band.sum() > 20 and (De[band] < 1e-100).all() and (Ds[band] > hu.MIN_WEIGHT).all() and (De[~band] > hu.MIN_WEIGHT).all()
    _is_the_constant(Lh, kp)
    gp, gq = _flat_guide(np.full((1, 2), 0.5, np.float32))[0], _flat_guide(np.full((1, 1), 0.5, np.float32))[0, 0]
    gp[1, 7] = 2000.0
    assert hu.edge(gp[0], gq, sigma) == 1 and hu.edge(gp[1], gq, sigma) == 0


def test_each_tier_alone():
    """opposed normals make w_n exactly 0 at every tap: the spatial tier everywhere.  Without any lo coverage neither tier divides: C = 0 and the pixel is its
    share of the background.  With kappa_p = 0 on the hi side e is 1 by vr_denoise.h's rule, whatever the normals."""
    f = 3
    L, kq, kp, B = _synthetic(7, 5, f)
    glo, ghi = _flat_guide(kq), _flat_guide(kp)
    glo[..., 4], ghi[..., 4] = 1.0, -1.0
    out, Lh = hu.upsample(L, glo, ghi, B, f)
    _, _, De, Ds = hu.spec_upsample(L, glo, ghi, B, f)
    assert (De[kp > 0] == 0).all() and (De[kp == 0] > hu.MIN_WEIGHT).all() and (Ds > hu.MIN_WEIGHT).all()
    _is_the_constant(Lh, kp)
    assert hu.min_weight() == hu.MIN_WEIGHT
    zero = np.zeros_like(L)
    out, Lh = hu.upsample(zero, _flat_guide(np.zeros_like(kq)), ghi, B, f)
    assert not Lh[..., :3].any() and _same(Lh[..., 3], kp) and _same(out[..., 3], kp)
    G = (np.float32(1) - kp)[..., None] * B[..., :3]
    assert _same(out[..., :3], np.float32(0) + G)


@pytest.mark.parametrize("w,h", ((1, 1), (2, 3)))
@pytest.mark.parametrize("f", (2, 3, 4))
def test_lo_frames_smaller_than_the_footprint(w, h, f):
    rs = np.random.RandomState(w + h + f)
    L, kq, kp, B = _synthetic(w, h, f, seed=w + 7 * f)
    L[..., :3] = rs.uniform(0.0, 2.0, (h, w, 3)) * kq[..., None]
    glo, ghi = _flat_guide(kq), _flat_guide(kp)
    glo[..., 0:3] = rs.uniform(0.3, 0.7, (h, w, 3))
    out, Lh = hu.upsample(L, glo, ghi, B, f)
    want_out, want_l, De, _ = hu.spec_upsample(L, glo, ghi, B, f)
    assert (De > hu.MIN_WEIGHT).all()
    assert np.isfinite(out).all() and np.abs(out - want_out).max() <= 2.0 ** -20 and np.abs(Lh - want_l).max() <= 2.0 ** -20
    if (w, h) == (1, 1):                             # one tap: C is the lo pixel's own colour whatever the weights
        with np.errstate(invalid="ignore"):
            assert np.abs(Lh[..., :3] - kp.astype(np.float64)[..., None] * (L[0, 0, :3].astype(np.float64) / kq[0, 0])).max() <= 2.0 ** -21


def test_the_split_the_fractions_and_the_spline():
    """x0 is the floor quotient (negative for the first hi pixels), r the remainder; at f = 2 the fractions are exactly 0.25 and 0.75; the weights are the
    cubic B-spline's to a few roundings, never negative (b_3 is 0 at a = 0, which odd factors reach), and sum to 1"""
    for f in (2, 3, 4):
        for x in range(0, 70):
            x0, r, a, b = hu.axis(x, f)
            assert (x0, r) == divmod(2 * x + 1 - f, 2 * f) and 0 <= r < 2 * f
            assert a == np.float32(r) / np.float32(2 * f)
            want = hu.spec_spline(float(a))
            assert np.abs(b - want).max() <= 4 * U and (b >= 0).all() and abs(float(b.astype(np.float64).sum()) - 1.0) <= 4 * U
            assert -1 <= x0 <= x // f
        assert hu.axis(0, f)[0] == -1
    assert [float(hu.axis(x, 2)[2]) for x in range(6)] == [0.75, 0.25, 0.75, 0.25, 0.75, 0.25]
    assert [hu.axis(x, 2)[0] for x in range(6)] == [-1, 0, 0, 1, 1, 2]


# ---- 3: the window the kernel stages ---------------------------------------------------------------------------------------------------------------------
# hi frames: one pixel; exactly one tile; ragged on both axes for every factor; several ragged tiles
WINDOW_FRAMES = ((2, 2), (16, 16), (72, 56), (72, 57), (132, 60))


@pytest.mark.parametrize("f", (2, 3, 4))
def test_the_scaled_window_holds_every_tap_where_the_kernel_looks(f):
    """ScaledTileWindow<f>: texel k of the window is the lo coordinate (x0 + k % kFoot, y0 + k / kFoot) -- how stage_window fills it -- and a thread finds tap
    (i, j) of its pixel at at(x0 - 1, y0 - 1) + j * kFoot + i -- how the kernel's accessor reads it -- inside the window, for every pixel of every tile,
    those outside a ragged frame included (their threads stage).  kFoot is 12, 9, 8: over these frames some tile's taps span all of it."""
    import hk_tiles
    span = 0
    for W, H in WINDOW_FRAMES:
        if W % f or H % f:
            W, H = W - W % f + f, H - H % f + f
        tx, ty, n = hk_tiles.grid(W, H)
        for tile in range(n):
            (foot, texels, wx0, wy0), first = hu.window(f, tile, W)
            assert foot == {2: 12, 3: 9, 4: 8}[f] and texels == foot * foot
            q = hk_tiles.pixels(tile, W)
            px, py = q[:, 3], q[:, 4]
            x0, y0 = np.floor_divide(2 * px + 1 - f, 2 * f), np.floor_divide(2 * py + 1 - f, 2 * f)
            assert np.array_equal(wx0 + first % foot, x0 - 1) and np.array_equal(wy0 + first // foot, y0 - 1)
            assert first.min() >= 0 and (first % foot + 3 < foot).all() and (first // foot + 3 < foot).all()      # the 4 x 4 taps stay in their rows and in the window
            assert wx0 == x0.min() - 1 and wy0 == y0.min() - 1                                                     # and the window starts at the first tap of any pixel
            span = max(span, int(x0.max() + 2 - wx0 + 1), int(y0.max() + 2 - wy0 + 1))
    assert span == {2: 12, 3: 9, 4: 8}[f]


# ---- 4: what it does to the error ----------------------------------------------------------------------------------------------------------------------
HI_W, HI_H = 128, 96
QUALITY = ("c2", "c3env", "c3", "c4_64", "c2hid")
COUNTS = (2, 4, 16)
MOST = {1: 16, 2: 64, 4: 256}                    # the samples traced per pixel at hi / f, once per process
# scene -> per n in COUNTS: (the unfiltered hi frame, today's best call, f = 2 at 4n spp, f = 4 at 16n spp), then the two sub-1-spp cells; measured with the
# host build (see test_the_error_at_equal_samples)
TABLE = {"c2": (((0.2718, 0.0626, 0.0363, 0.0331), (0.1974, 0.0397, 0.0285, 0.0290), (0.0993, 0.0283, 0.0247, 0.0254)), (0.0378, 0.0296)),
         "c3env": (((0.1391, 0.0168, 0.0123, 0.0142), (0.0950, 0.0129, 0.0120, 0.0137), (0.0469, 0.0100, 0.0109, 0.0128)), (0.0134, 0.0123)),
         "c3": (((1.8594, 0.4018, 0.3036, 0.3288), (1.3071, 0.3114, 0.2835, 0.3178), (0.6231, 0.2286, 0.2465, 0.2917)), (0.3231, 0.2839)),
         "c4_64": (((0.3630, 0.0806, 0.0577, 0.0529), (0.2521, 0.0577, 0.0502, 0.0401), (0.1272, 0.0354, 0.0361, 0.0335)), (0.0593, 0.0511)),
         "c2hid": (((0.8951, 0.1757, 0.1109, 0.0980), (0.6443, 0.1157, 0.0868, 0.0845), (0.3185, 0.0859, 0.0745, 0.0756)), (0.1106, 0.0903))}
GUARD = 1.1                                      # a recorded cell may not grow past this: the seed-to-seed spread tests/test_layers_host.py allows itself


def _resolved(name, spp, f):
    w, h = HI_W // f, HI_H // f
    fb, var = trh._inputs(name, spp, w, h, MOST[f])
    feat = trh._guide(name, w, h)
    y, B = hr.resolved(trh._oracle(name, w, h), RAYS, fb, feat)
    return fb, y, B, var, feat


def _sub_one_spp(name, spp, ghi, Bh):
    """8 frames of spp samples at 64x48 (frame k = samples spp k + 1 .. spp k + spp of the run of seed 42), fixed camera, "denoise_moments" = 1, alpha 0.2:
    the last frame's layer upsampled by 2"""
    from test_gpu_features import _replay
    trh._inputs(name, 2, HI_W // 2, HI_H // 2, MOST[2])
    radiance = trh._RADIANCE[name, HI_W // 2, HI_H // 2, MOST[2]]
    o, feat = trh._oracle(name, HI_W // 2, HI_H // 2), trh._guide(name, HI_W // 2, HI_H // 2)
    p = o.params()
    cam = ht.camera(list(p.cam_pos), list(p.cam_transform), fov_degree=float(p.cam_fov))
    replay = hl.Replay(moments=True)
    for k in range(8):
        mu, S = _replay(radiance[spp * k:spp * k + spp])
        var = (S * (np.float32(spp) / np.float32(spp - 1))).astype(np.float32) if spp >= 2 else np.zeros_like(S)
        y, B = hr.resolved(o, RAYS, mu, feat)
        L = replay.frame(cam, y, B, var, feat, spp, 0.2)[4]
    return hu.upsample(L, hu.guide(feat), ghi, Bh, 2)[0]


@pytest.mark.parametrize("name", QUALITY)
def test_the_error_at_equal_samples(name):
    """Oracle frames of seed 42, hi 128x96, 2 x 2 expected rays, default sigmas; relative L2 of RGB over the whole hi frame against 1024 spp at 128x96 of seed
    1234567.  c3env = c3 with show_environment 1, c2hid = c2 with show_environment 0.  Per n: the unfiltered hi frame of n spp; today's best call (n spp at
    128x96, denoise_layers on); this call, 4n spp at 64x48 layered and upsampled by 2; 16n spp at 32x24 upsampled by 4.  Measured with the host build:
                 n = 2: raw     best    f = 2   f = 4     n = 4: raw     best    f = 2   f = 4     n = 16: raw    best    f = 2   f = 4
      c2                0.2718  0.0626  0.0363  0.0331           0.1974  0.0397  0.0285  0.0290            0.0993  0.0283  0.0247  0.0254
      c3env             0.1391  0.0168  0.0123  0.0142           0.0950  0.0129  0.0120  0.0137*           0.0469  0.0100  0.0109* 0.0128*
      c3                1.8594  0.4018  0.3036  0.3288           1.3071  0.3114  0.2835  0.3178*           0.6231  0.2286  0.2465* 0.2917*
      c4_64             0.3630  0.0806  0.0577  0.0529           0.2521  0.0577  0.0502  0.0401            0.1272  0.0354  0.0361* 0.0335
      c2hid             0.8951  0.1757  0.1109  0.0980           0.6443  0.1157  0.0868  0.0845            0.3185  0.0859  0.0745  0.0756
    (*: loses to today's best call.)  Below one sample per hi pixel -- 8 frames of 1 and of 2 spp at 64x48 with denoise_moments, upsampled by 2, i.e. 0.25 and
    0.5 spp per hi pixel and frame: c2 0.0378 0.0296, c3env 0.0134 0.0123, c3 0.3231 0.2839, c4_64 0.0593 0.0511, c2hid 0.1106 0.0903.
    Asserted: no recorded cell grows past 1.1 x its value; every upsampled cell beats the unfiltered hi frame of equal samples, as the table says all do;
    and where the table says f = 2 beats today's best call it still does."""
    ref = trh._oracle(name, HI_W, HI_H, seed=1234567).render(1024)[..., :3]
    ghi, Bh = _hi(name, HI_W, HI_H)
    rows = []
    for n in COUNTS:
        fb, y, B, var, feat = _resolved(name, n, 1)
        cells = [scenes.rel_l2(fb[..., :3], ref), scenes.rel_l2(hl.layered(y, B, var, feat, n)[0][..., :3], ref)]
        for f in (2, 4):
            _, y, B, var, feat = _resolved(name, n * f * f, f)
            L = hl.layered(y, B, var, feat, n * f * f)[1]
            cells.append(scenes.rel_l2(hu.upsample(L, hu.guide(feat), ghi, Bh, f)[0][..., :3], ref))
        rows.append(cells)
    sub = [scenes.rel_l2(_sub_one_spp(name, spp, ghi, Bh)[..., :3], ref) for spp in (1, 2)]
    print("%-6s %s   sub %s" % (name, "   ".join("n=%d: %s" % (n, " ".join("%.4f" % c for c in cells)) for n, cells in zip(COUNTS, rows)), " ".join("%.4f" % c for c in sub)))
    want_rows, want_sub = TABLE[name]
    for n, cells, want in zip(COUNTS, rows, want_rows):
        for got, rec in zip(cells, want):
            assert np.isfinite(got) and got <= GUARD * rec, (name, n, got, rec)
        raw, best, f2, f4 = cells
        assert f2 < raw and f4 < raw, (name, n, cells)
        if want[2] < want[1]:
            assert f2 < best, (name, n, cells)
    for got, rec in zip(sub, want_sub):
        assert np.isfinite(got) and got <= GUARD * rec, (name, got, rec)
