"""CPU: the layered filter (volren_amd/csrc/vr_layers.h) built for the host (tests/hostkernel/layers_host.cpp): its split and merge against a float64 numpy
statement of the header (tests/hk_layers.py) on oracle frames; its identities on synthetic frames; what it does to the error of oracle frames next to
today's best call, the filter on the resolved frame; and a temporal sequence.  tests/test_gpu_layers.py holds the HIP kernels to this build bit for bit.
The frames, guides and references are tests/test_resolve_host.py's own, traced once per process."""
import numpy as np
import pytest

import hk_denoise
import hk_expected as he
import hk_layers as hl
import hk_resolve as hr
import hk_temporal as ht
import scenes
import test_resolve_host as trh
from hk_common import same as _same

W, H, RAYS = trh.W, trh.H, trh.RAYS
SCENES = trh.SCENES


def _resolved(name, spp, w=W, h=H, most=64):
    """(y, B, var, guide) of the oracle frame of seed 42"""
    fb, var = trh._inputs(name, spp, w, h, most)
    guide = trh._guide(name, w, h)
    y, B = hr.resolved(trh._oracle(name, w, h), RAYS, fb, guide)
    return y, B, var, guide


# ---- 1: the host build is the header ------------------------------------------------------------------------------------------------------------------
# largest |host - float64 statement| per channel over both frame sizes, recorded from the host build; asserted at 4x
# (tests/test_filter_cases_host.py holds crafted frames of larger values to these too, times magnitude / the magnitude measured here: its _scaled)
# (S, out, L)
RECORDED = {"c2": ((3.84e-8, 4.76e-8, 4.54e-8), (6.33e-8, 5.49e-8, 6.69e-8), (3.85e-8, 3.27e-8, 2.83e-8)),
            "c3env": ((4.02e-8, 4.29e-8, 4.28e-8), (5.58e-8, 6.93e-8, 5.77e-8), (7.37e-9, 5.15e-9, 6.59e-9)),
            "c4_64": ((1.00e-7, 1.16e-7, 1.12e-7), (1.29e-7, 1.42e-7, 1.48e-7), (6.87e-8, 6.67e-8, 5.24e-8))}


@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_matches_the_float64_statement(name):
    """Frames of 8 spp at 64x48 and 48x32 against 2 x 2 expected rays: S against hk_layers.spec_split of the host's y and B, out and L against
    hk_layers.spec_merge of the host filter's F.  Each is two or three float32 roundings of values below 4; the alphas are kappa bit for bit."""
    worst = np.zeros((3, 3))
    for w, h in ((64, 48), (48, 32)):
        y, B, var, guide = _resolved(name, 8, w, h, most=64 if (w, h) == (W, H) else 8)
        kappa = guide[..., 3]
        out, L, S, F = hl.layered(y, B, var, guide, 8)
        assert np.isfinite(out).all() and np.isfinite(L).all() and (out[..., :3] >= 0).all()
        assert _same(S[..., 3], kappa) and _same(L[..., 3], kappa) and _same(out[..., 3], kappa)
        want_out, want_l = hl.spec_merge(F, B, kappa)
        for i, (got, want) in enumerate(((S, hl.spec_split(y, B, kappa)), (out, want_out), (L, want_l))):
            worst[i] = np.maximum(worst[i], np.abs(got - want)[..., :3].max(axis=(0, 1)))
        assert not _same(out, hk_denoise.denoise(y, var, guide, 8))
    print("%s: S %s   out %s   L %s" % ((name,) + tuple(" ".join("%.3g" % x for x in row) for row in worst)))
    assert (worst <= 4 * np.array(RECORDED[name])).all()


# ---- 2: identities ---------------------------------------------------------------------------------------------------------------------------------------
def _flat_guide(kappa):
    """a guide that stops the filter nowhere but on the coverage: one albedo, no normal, one depth"""
    h, w = kappa.shape
    g = np.zeros((h, w, 8), np.float32)
    g[..., 0:3] = 0.5
    g[..., 3] = kappa
    g[..., 7] = 2.0
    return g


def test_pixels_without_coverage_give_the_background_bit_for_bit():
    """on an oracle frame (the sky around c3env's volume: at 64x48 the five iterations reach it from every pixel) and on a synthetic F; a filtered coverage
    of 2^-20 or less leaves F.rgb as it is"""
    y, B, var, guide = _resolved("c3env", 8)
    out, L, _, F = hl.layered(y, B, var, guide, 8)
    none = guide[..., 3] == 0
    assert none.sum() > 500 and (F[..., 3][none] > hl.MIN_WEIGHT).any() and np.abs(F[..., :3][none]).max() > 1e-3      # (the filter did find light around them)
    assert _same(out[none][:, :3], B[none][:, :3]) and not np.abs(L[none]).any()
    assert not _same(y[none][:, :3], B[none][:, :3])                      # (the frame's sky is sampled, B's is the quadrature)
    rs = np.random.RandomState(3)
    F = rs.uniform(-2.0, 2.0, (7, 9, 4)).astype(np.float32)
    F[..., 3] = rs.choice(np.array([2.0 ** -20 * (1 + 2.0 ** -23), 2.0 ** -19, 0.5], np.float32), (7, 9))
    Bs = np.zeros((7, 9, 4), np.float32)
    Bs[..., :3] = rs.uniform(0.0, 3.0, (7, 9, 3))
    out, L = hl.merge(F, Bs, np.zeros((7, 9), np.float32))
    assert _same(out[..., :3], Bs[..., :3]) and not np.abs(L).any() and not out[..., 3].any()
    assert hl.min_weight() == hl.MIN_WEIGHT
    F[..., 3] = rs.choice(np.array([0.0, 2.0 ** -21, 2.0 ** -20], np.float32), (7, 9))
    kappa = rs.uniform(0.0, 1.0, (7, 9)).astype(np.float32)
    kappa[0] = 0
    out, L = hl.merge(F, Bs, kappa)
    assert _same(L[..., :3], F[..., :3]) and _same(L[..., 3], kappa)


def test_zero_iterations_give_the_resolved_frame():
    """F = S: the ratio is 1 and out = max(0, G + (y - G)), y to two roundings of values below 4 (2^-22 each at most)"""
    for name in ("c2", "c3env"):
        y, B, var, guide = _resolved(name, 8)
        out, L, S, F = hl.layered(y, B, var, guide, 8, iterations=0)
        assert _same(F, S) and _same(L, S)
        small = (y[..., :3] < 4).all(axis=-1) & (B[..., :3] < 4).all(axis=-1)
        assert small.mean() > 0.9 and np.abs(out - np.maximum(y, 0))[small].max() <= 2.0 ** -21


def _ramp(w=40, h=24, seed=9):
    """x = (1 - kappa) B + kappa C: C constant, kappa a ramp across the frame, B a random texture in [0, 3]; a variance of 0.25 everywhere"""
    rs = np.random.RandomState(seed)
    kappa = np.tile(np.linspace(0.0, 1.0, w, dtype=np.float32), (h, 1))
    B = np.zeros((h, w, 4), np.float32)
    B[..., :3] = rs.uniform(0.0, 3.0, (h, w, 3))
    Cc = np.array([0.3, 0.7, 0.45])
    k64 = kappa.astype(np.float64)[..., None]
    x = np.concatenate([(1.0 - k64) * B[..., :3] + k64 * Cc, k64], axis=2).astype(np.float32)
    return x, B, kappa, np.full((h, w, 4), 0.25, np.float32)


def test_a_ramp_of_coverage_over_a_textured_background_comes_back_as_itself():
    """every pixel's F.rgb / F.a is C whatever the weights, so the merge gives (1 - kappa) B + kappa C back: to 2^-20 (G, the sum and x's own rounding are
    2^-23 each on values below 4; C F.a / F.a costs the filter's 5 x 25 sums at a relative 2^-24 each on C < 1).  The plain filter on the same frame blurs B."""
    x, B, kappa, var = _ramp()
    guide = _flat_guide(kappa)
    out, _, _, _ = hl.layered(x, B, var, guide, 4)
    plain = hk_denoise.denoise(x, var, guide, 4)
    print("layered moves the frame by %.3g, the plain filter by %.3g" % (np.abs(out - x).max(), np.abs(plain - x)[..., :3].max()))
    assert np.abs(out - x).max() <= 2.0 ** -20
    assert np.abs(plain - x)[..., :3].max() > 0.01


def test_a_hidden_environment_leaves_the_renormalised_layer():
    for name in ("c3", "c2hid"):
        o = trh._oracle(name, 32, 24)
        fb = o.render(4)
        guide = he.expected_pass(o, RAYS)
        y, B = hr.resolved(o, RAYS, fb, guide)
        var = np.full((24, 32, 4), 0.01, np.float32)
        out, L, S, F = hl.layered(y, B, var, guide, 4)
        kappa = guide[..., 3]
        assert not B.any() and _same(S[..., :3], y[..., :3])                          # G = 0
        big = F[..., 3] > hl.MIN_WEIGHT
        assert big.sum() > 100
        with np.errstate(divide="ignore", invalid="ignore"):
            want = (F[..., :3] * (kappa / F[..., 3])[..., None]).astype(np.float32)
        t = np.float32(0) + want[big]
        assert _same(L[big][:, :3], want[big]) and _same(out[big][:, :3], np.where(t < 0, np.float32(0), t))


@pytest.mark.parametrize("w,h", ((1, 1), (3, 3), (2, 9)))
def test_frames_smaller_than_the_filter(w, h):
    rs = np.random.RandomState(w + h)
    y = rs.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    B = np.zeros((h, w, 4), np.float32)
    B[..., :3] = rs.uniform(0.0, 3.0, (h, w, 3))
    kappa = rs.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    kappa[0, 0] = 0.0
    var = rs.uniform(0.0, 0.5, (h, w, 4)).astype(np.float32)
    out, L, S, F = hl.layered(y, B, var, _flat_guide(kappa), 4)
    want_out, want_l = hl.spec_merge(F, B, kappa)
    assert np.isfinite(out).all() and np.abs(out - want_out).max() <= 2.0 ** -20 and np.abs(L - want_l).max() <= 2.0 ** -20
    if F[0, 0, 3] > hl.MIN_WEIGHT:                   # (kappa = 0 there; in a frame of one pixel nothing covered is in reach and the pixel is y again)
        assert _same(out[0, 0, :3], B[0, 0, :3])
    else:
        assert (w, h) == (1, 1) and np.abs(out[0, 0, :3] - y[0, 0, :3]).max() <= 2.0 ** -21
    o = trh._oracle("c2", w, h)
    guide = he.expected_pass(o, RAYS)
    yo, Bo = hr.resolved(o, RAYS, o.render(4), guide)
    assert np.isfinite(hl.layered(yo, Bo, np.full((h, w, 4), 0.1, np.float32), guide, 4)[0]).all()


# ---- 3: what it does to the error --------------------------------------------------------------------------------------------------------------------
SPPS = (2, 4, 16, 64)
# scene -> the factor layered / denoise(y) may reach at each of SPPS (None: recorded only; "skip": not run)
ASSERTED = {"c3env": (0.5, 0.5, 0.5, 0.5), "c2": (0.9, 0.9, 0.9, 0.9), "c2hid": (0.9, "skip", 0.9, 0.9), "c4_64": (None, None, 1.0, 1.0), "c3": (None,) * 4}


def _cells(name, spp):
    y, B, var, guide = _resolved(name, spp)
    ref = trh._reference(name)
    return (scenes.rel_l2(hk_denoise.denoise(y, var, guide, spp)[..., :3], ref), scenes.rel_l2(hl.layered(y, B, var, guide, spp)[0][..., :3], ref),
            scenes.rel_l2(y[..., :3], ref))


@pytest.mark.parametrize("name", sorted(ASSERTED))
def test_the_error_next_to_the_filter_on_the_resolved_frame(name):
    """Oracle frames at 64x48 of seed 42 (samples 1..n of one run), 2 x 2 expected rays, default sigmas, the frame's own variance; relative L2 of RGB over the
    whole frame against 1024 spp of seed 1234567.  c3env = c3 with show_environment 1, c2hid = c2 with show_environment 0.  Measured with the product's float32
    split and merge (denoise with denoise_resolve = 1 -> the layered result):
                 2 spp              4 spp              16 spp             64 spp
      c3env      0.0695 -> 0.0207   0.0557 -> 0.0156   0.0403 -> 0.0122   0.0294 -> 0.0106
      c2         0.0959 -> 0.0765   0.0735 -> 0.0555   0.0487 -> 0.0314   0.0380 -> 0.0257
      c4_64      0.1026 -> 0.0978   0.0814 -> 0.0755   0.0579 -> 0.0514   0.0425 -> 0.0360
      c2hid      0.2810 -> 0.2221   not run            0.1539 -> 0.0951   0.1191 -> 0.0784
      c3         0.5894 -> 0.6167   0.4004 -> 0.3919   0.2867 -> 0.2585   0.2139 -> 0.1981
    The unfiltered resolved frame of c3env has 0.0727, 0.0535, 0.0301 and 0.0151.
    Asserted: c3env layered <= 0.5 x at all four counts; c2 <= 0.9 x at all four; c2hid <= 0.9 x at 2, 16 and 64 spp; c4_64 <= 1.0 x at 16 and 64 spp; on c3env
    at 16 and 64 spp layered <= the unfiltered resolved frame.  c4_64 at 2 and 4 spp and all of c3 are recorded only: c3 at 2 spp loses."""
    cells = {spp: _cells(name, spp) for spp, bound in zip(SPPS, ASSERTED[name]) if bound != "skip"}
    print("%-6s %s" % (name, "   ".join("%3d spp %.4f -> %.4f (y %.4f)" % ((spp,) + cells[spp]) for spp in cells)))
    for spp, bound in zip(SPPS, ASSERTED[name]):
        if bound == "skip":
            continue
        base, lay, raw = cells[spp]
        assert np.isfinite(base) and np.isfinite(lay)
        if bound is not None:
            assert lay <= bound * base, (name, spp, base, lay, bound)
        if name == "c3env" and spp in (16, 64):
            assert lay <= raw, (spp, lay, raw)


def test_the_partially_covered_pixels_of_c3_with_the_sky_shown():
    """Restricted to the 446 pixels with 0.02 < kappa < 0.98: 0.1535 -> 0.0554 at 2 spp, 0.0589 -> 0.0288 at 64 spp (measured); asserted at the whole frame's bound, layered <= 0.5 x"""
    ref, guide = trh._reference("c3env"), trh._guide("c3env")
    m = (guide[..., 3] > 0.02) & (guide[..., 3] < 0.98)
    for spp in (2, 64):
        y, B, var, _ = _resolved("c3env", spp)
        base = scenes.rel_l2(hk_denoise.denoise(y, var, guide, spp)[..., :3][m], ref[m])
        lay = scenes.rel_l2(hl.layered(y, B, var, guide, spp)[0][..., :3][m], ref[m])
        print("c3env, %d pixels with 0.02 < kappa < 0.98, %d spp: %.4f -> %.4f" % (int(m.sum()), spp, base, lay))
        assert lay <= 0.5 * base


# ---- 4: temporal -----------------------------------------------------------------------------------------------------------------------------------------
ALPHA = ht.constants()[0]                        # the default of "denoise_alpha"


def _camera(o):
    p = o.params()
    return ht.camera(list(p.cam_pos), list(p.cam_transform), fov_degree=float(p.cam_fov))


def _sequence(frames):
    """frames: (camera, y, B, var, guide) each, of 2 spp -> the last results of the filter on y (denoise_resolve alone) and of the layered filter"""
    plain, layered = ht.Replay(), hl.Replay()
    for cam, y, B, var, guide in frames:
        a = plain.frame(cam, y, var, guide, 2, ALPHA)[3]
        b = layered.frame(cam, y, B, var, guide, 2, ALPHA)[3]
    return a, b


def test_eight_frames_of_2_spp_under_a_fixed_camera():
    """c3env, frame k = samples 2k + 1, 2k + 2 of the run of seed 42 (independent paths), alpha 0.2: the last frame's error, 0.0401 -> 0.0122 (measured,
    denoise_resolve alone -> layered); asserted layered <= denoise_resolve alone"""
    from test_gpu_features import _replay
    trh._inputs("c3env", 2)
    L = trh._RADIANCE["c3env", W, H, 64]
    o, guide = trh._oracle("c3env"), trh._guide("c3env")
    frames = []
    for k in range(8):
        mu, S = _replay(L[2 * k:2 * k + 2])
        y, B = hr.resolved(o, RAYS, mu, guide)
        frames.append((_camera(o), y, B, (S * np.float32(2)).astype(np.float32), guide))
    a, b = _sequence(frames)
    ref = trh._reference("c3env")
    ea, eb = scenes.rel_l2(a[..., :3], ref), scenes.rel_l2(b[..., :3], ref)
    print("c3env, 8 frames of 2 spp, fixed camera: %.4f -> %.4f" % (ea, eb))
    assert eb <= ea


def test_eight_frames_of_2_spp_under_a_turning_camera_are_recorded():
    """the same with the camera on an orbit about the volume, 1 degree per frame (seed 42 + k per frame), against 256 spp of seed 1234567 from the last camera:
    0.0532 -> 0.0170 (measured, denoise_resolve alone -> layered).  Nothing is asserted but that both are finite."""
    from gpu_frames import _orbit
    from test_gpu_features import _replay
    frames = []
    for k in range(8):
        o = trh._oracle("c3env", seed=42 + k)
        _orbit(o, float(k))
        mu, S = _replay(trh._radiance(o, 2))
        guide = he.expected_pass(o, RAYS)
        y, B = hr.resolved(o, RAYS, mu, guide)
        frames.append((_camera(o), y, B, (S * np.float32(2)).astype(np.float32), guide))
    a, b = _sequence(frames)
    o = trh._oracle("c3env", seed=1234567)
    _orbit(o, 7.0)
    ref = o.render(256)[..., :3]
    ea, eb = scenes.rel_l2(a[..., :3], ref), scenes.rel_l2(b[..., :3], ref)
    print("c3env, 8 frames of 2 spp, 1 degree per frame: %.4f -> %.4f" % (ea, eb))
    assert np.isfinite(ea) and np.isfinite(eb)
