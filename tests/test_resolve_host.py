"""CPU: the control variate on the expected coverage (volren_amd/csrc/vr_resolve.h) built for the host (tests/hostkernel/resolve_host.cpp): against a
float64 numpy statement of the header (tests/hk_resolve.py) on oracle frames; its identities on synthetic frames; what it does to the error of oracle
frames, raw and through the filter; and its bias at 1024 spp.  tests/test_gpu_resolve.py holds the HIP kernels to this build bit for bit."""
import numpy as np
import pytest

import hk_denoise
import hk_expected as he
import hk_resolve as hr
import scenes
from hk_common import same as _same

W, H, RAYS = 64, 48, 2
SCENES = ("c2", "c3env", "c4_64")                # smoke.brick in front of the sky; the same under the LUT with the sky shown; a dense fp16 grid


def _oracle(name, w=W, h=H, seed=42):
    o = scenes.oracle_scene({"c3env": "c3", "c2hid": "c2"}.get(name, name), w, h)
    if name == "c3env":
        o.show_environment = True
    if name == "c2hid":
        o.show_environment = False
    o.seed = seed
    return o


_GUIDE, _RADIANCE, _FRAME = {}, {}, {}


def _guide(name, w=W, h=H):
    if (name, w, h) not in _GUIDE:
        _GUIDE[name, w, h] = he.expected_pass(_oracle(name, w, h), RAYS)
    return _GUIDE[name, w, h]


def _inputs(name, spp, w=W, h=H, most=64):
    """(mean, unbiased variance) of samples 1..spp of an oracle frame of seed 42: the per-sample radiances (traced once, for the `most` samples any caller
    asks for) replayed through the accumulation pass's arithmetic (test_gpu_features._replay)"""
    from test_gpu_features import _replay
    assert 2 <= spp <= most
    if (name, w, h, most) not in _RADIANCE:
        _RADIANCE[name, w, h, most] = _radiance(_oracle(name, w, h), most)
    mu, S = _replay(_RADIANCE[name, w, h, most][:spp])
    return mu, (S * (np.float32(spp) / np.float32(spp - 1))).astype(np.float32)


def _radiance(o, spp):
    """test_gpu_features._oracle_radiance, the rows spread over a few threads (the oracle's per-sample call keeps its state on its own stack)"""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor

    from oracle import binding as ob
    p, s, fn = o.params(), o.scene(), ob.lib().orc_trace_pixel_sample
    L = np.zeros((spp, o.h, o.w, 4), np.float32)

    def row(y):
        out = np.zeros(4, np.float32)
        ptr = ob.fptr(out)
        for x in range(o.w):
            for k in range(spp):
                fn(C.byref(p), C.byref(s), x, y, k + 1, ptr)
                L[k, y, x] = out
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(row, range(o.h)))
    return L


def _frame(name, spp, seed=42):
    if (name, spp, seed) not in _FRAME:
        _FRAME[name, spp, seed] = _oracle(name, seed=seed).render(spp).copy()
    return _FRAME[name, spp, seed]


# ---- 1: the host build is the header ------------------------------------------------------------------------------------------------------------------
# largest |host - float64 statement| per channel over both frame sizes, recorded from the host build; asserted at 4x
# (tests/test_filter_cases_host.py holds crafted frames of larger values to these too, times magnitude / the magnitude measured here: its _scaled)
RECORDED = {"c2": ((2.01e-6, 2.73e-6, 2.45e-6), (5.56e-8, 4.10e-8, 3.27e-8)),
            "c3env": ((2.01e-6, 2.73e-6, 2.45e-6), (3.18e-8, 3.70e-8, 2.93e-8)),
            "c4_64": ((2.03e-6, 1.36e-6, 2.24e-6), (1.12e-7, 8.06e-8, 1.07e-7))}


@pytest.mark.parametrize("name", SCENES)
def test_the_host_build_matches_the_float64_statement(name):
    """Frames of 8 spp at 64x48 and 48x32 against 2 x 2 expected rays: B against hk_resolve.spec_background (the sub-ray directions, the inverse
    transform, the equirectangular lookup with its bilinear fetch, the strength, in float64), y against hk_resolve.spec_resolve fed with the host's B.
    B's difference is the float32 rounding of (u, v) times 1024 x 512 texels times the sky's gradient; y's is a few roundings of a value below 2.  The
    filter behind it takes the frame's variance untouched: the host filter on y is the iterations started from (y, prepare(the frame's variance))."""
    worst_b, worst_y = np.zeros(3), np.zeros(3)
    for w, h in ((64, 48), (48, 32)):
        o = _oracle(name, w, h)
        fb, var = _inputs(name, 8, w, h, most=64 if (w, h) == (W, H) else 8)
        guide = _guide(name, w, h)
        y, B = hr.resolved(o, RAYS, fb, guide)
        assert np.isfinite(y).all() and (B[..., :3] > 0).all() and not B[..., 3].any()
        assert _same(y[..., 3], guide[..., 3])
        worst_b = np.maximum(worst_b, np.abs(B[..., :3] - hr.spec_background(o, RAYS)).max(axis=(0, 1)))
        worst_y = np.maximum(worst_y, np.abs(y - hr.spec_resolve(fb, B, guide[..., 3]))[..., :3].max(axis=(0, 1)))
        v, g = hk_denoise.prepare(var, guide, 8)
        c = y
        for k in range(5):
            c, v = hk_denoise.atrous(c, v, g, 1 << k)
        assert _same(c, hk_denoise.denoise(y, var, guide, 8)) and not _same(c, hk_denoise.denoise(fb, var, guide, 8))
    print("%s: B %s   y %s" % (name, " ".join("%.3g" % x for x in worst_b), " ".join("%.3g" % x for x in worst_y)))
    rec_b, rec_y = RECORDED[name]
    assert (worst_b <= 4 * np.array(rec_b)).all() and (worst_y <= 4 * np.array(rec_y)).all()


# ---- 2: identities ---------------------------------------------------------------------------------------------------------------------------------------
def _synthetic(w, h, seed=5):
    rs = np.random.RandomState(seed)
    fb = rs.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    fb[..., 3] = rs.randint(0, 9, (h, w)).astype(np.float32) / np.float32(8)             # shares of 8 samples
    B = np.zeros((h, w, 4), np.float32)
    B[..., :3] = rs.uniform(0.0, 3.0, (h, w, 3))
    return fb, B, rs.uniform(0.0, 1.0, (h, w)).astype(np.float32)


def test_equal_coverages_give_the_frame_back_bit_for_bit():
    fb, B, _ = _synthetic(23, 17)
    y = hr.resolve(fb, B, hr.part(fb, B), fb[..., 3])
    assert _same(y, fb)


def test_a_two_valued_frame_resolves_to_its_expectation():
    """x = (1 - k^) B + k^ C with constant B and C and random k^, k: every pixel's C~ is C, so y = (1 - k) B + k C up to the rounding of a handful of
    float32 operations on values below 4 (2^-21 absolute allows 8 of them)"""
    rs = np.random.RandomState(11)
    h, w = 19, 26
    Bc, Cc = np.array([3.0, 0.5, 1.25]), np.array([0.25, 2.0, 1.0])
    kh = rs.randint(0, 5, (h, w)) / 4.0
    kh[0, 0] = 1.0                                                    # (at least one hit in the frame)
    k = rs.uniform(0.0, 1.0, (h, w))
    fb = np.concatenate([(1 - kh)[..., None] * Bc + kh[..., None] * Cc, kh[..., None]], axis=2).astype(np.float32)
    B = np.zeros((h, w, 4), np.float32)
    B[..., :3] = Bc
    k32 = k.astype(np.float32)
    y = hr.resolve(fb, B, hr.part(fb, B), k32)
    hit = hr._window_sum(kh[..., None])[..., 0] > 0
    want = (1 - k32.astype(np.float64))[..., None] * Bc + k32.astype(np.float64)[..., None] * Cc
    assert hit.sum() > 400 and np.abs(y[..., :3] - want)[hit].max() <= 2.0 ** -21
    assert _same(y[..., 3], k32)


def test_a_window_without_a_hit_takes_the_background_as_coefficient():
    """no sample hit anywhere: D = 0, C~ = 0, beta = B, and the frame is B itself: y = B + B (0 - k), not below 0"""
    fb, B, k = _synthetic(12, 9)
    fb[..., 3] = 0
    fb[..., :3] = B[..., :3]
    y = hr.resolve(fb, B, hr.part(fb, B), k)
    want = np.maximum((B[..., :3] + (B[..., :3] * (np.float32(0) - k)[..., None]).astype(np.float32)).astype(np.float32), 0)
    assert _same(y[..., :3], want) and _same(y[..., 3], k) and (y[..., :3] < B[..., :3]).any()
    assert _same(hr.part(fb, B)[..., :3], np.zeros((9, 12, 3), np.float32))


@pytest.mark.parametrize("w,h", ((1, 1), (3, 3), (2, 9)))
def test_frames_smaller_than_the_window(w, h):
    fb, B, k = _synthetic(w, h, seed=w + h)
    fb[0, 0, 3] = 0.5
    y = hr.resolve(fb, B, hr.part(fb, B), k)
    assert np.abs(y - hr.spec_resolve(fb, B, k)).max() <= 2.0 ** -20 and np.isfinite(y).all()
    o = _oracle("c2", w, h)
    yo, Bo = hr.resolved(o, RAYS, o.render(4), he.expected_pass(o, RAYS))
    assert np.isfinite(yo).all() and (Bo[..., :3] > 0).all()


def test_a_hidden_environment_gives_no_background():
    for name in ("c3", "c2hid"):
        o = _oracle(name, 32, 24)
        assert not o.show_environment
        fb = o.render(4)
        y, B = hr.resolved(o, RAYS, fb, he.expected_pass(o, RAYS))
        assert not B.any() and np.isfinite(y).all() and not _same(y, fb)
        assert not hr.spec_background(o, RAYS).any()


# ---- 3: what it does to the error --------------------------------------------------------------------------------------------------------------------
_REFERENCE = {}


def _reference(name):
    if name not in _REFERENCE:
        _REFERENCE[name] = _oracle(name, seed=1234567).render(1024).copy()[..., :3]
    return _REFERENCE[name]


def _cells(name, spp, filtered):
    ref, guide = _reference(name), _guide(name)
    if filtered or name != "c2hid":
        fb, var = _inputs(name, spp)
    else:
        fb, var = _frame(name, spp), None
    y, _ = hr.resolved(_oracle(name), RAYS, fb, guide)
    if filtered:
        return scenes.rel_l2(hk_denoise.denoise(fb, var, guide, spp)[..., :3], ref), scenes.rel_l2(hk_denoise.denoise(y, var, guide, spp)[..., :3], ref)
    return scenes.rel_l2(fb[..., :3], ref), scenes.rel_l2(y[..., :3], ref)


SPPS = (2, 4, 16, 64)
# (scene, filtered) -> the factor resolved / raw may reach at each of SPPS (None: recorded only)
ASSERTED = {("c3env", False): (0.75, 0.75, 0.75, 0.75), ("c3env", True): (0.95, 0.95, 0.95, None),
            ("c2", False): (1.0, 1.0, 1.0, None), ("c2", True): (None,) * 4,
            ("c4_64", False): (1.0, 1.0, None, None), ("c4_64", True): (None,) * 4,
            ("c2hid", False): (None,) * 4}


@pytest.mark.parametrize("name,filtered", sorted(ASSERTED))
def test_the_error_of_oracle_frames_before_and_after(name, filtered):
    """Oracle frames at 64x48 of seed 42 (samples 1..n of one run) resolved against 2 x 2 expected rays, relative L2 of RGB over the whole frame against
    1024 spp of seed 1234567; "filtered": both frames through the host filter at default sigmas with the expected guide and the frame's own variance.
    c3env = c3 with show_environment 1, c2hid = c2 with show_environment 0.  Measured with the product's float32 arithmetic and its own B (frame -> resolved):
                         2 spp              4 spp              16 spp             64 spp
      c3env  raw         0.1323 -> 0.0727   0.0910 -> 0.0535   0.0472 -> 0.0301   0.0249 -> 0.0151
      c3env  filtered    0.0849 -> 0.0695   0.0648 -> 0.0557   0.0456 -> 0.0403   0.0326 -> 0.0294
      c2     raw         0.2934 -> 0.2829   0.2091 -> 0.2029   0.0988 -> 0.0959   0.0530 -> 0.0523
      c2     filtered    0.1012 -> 0.0959   0.0757 -> 0.0735   0.0495 -> 0.0487   0.0382 -> 0.0380
      c4_64  raw         0.3574 -> 0.3502   0.2527 -> 0.2490   0.1303 -> 0.1283   0.0659 -> 0.0656
      c4_64  filtered    0.1088 -> 0.1026   0.0833 -> 0.0814   0.0584 -> 0.0579   0.0418 -> 0.0425
      c2hid  raw         0.9306 -> 0.8600   0.6651 -> 0.6282   0.3192 -> 0.2966   0.1731 -> 0.1647
    Asserted, with the margins of the float64 prototype's ratios (0.55 - 0.64 raw and 0.82 - 0.88 filtered on c3env): c3env raw at all four counts
    resolved <= 0.75 x raw; c3env filtered at 2, 4 and 16 spp resolved <= 0.95 x raw; c2 raw at 2, 4 and 16 spp and c4_64 raw at 2 and 4 spp resolved <=
    raw.  The other cells are recorded only: their margins are below 1 %, and one of them (c4_64 filtered at 64 spp) is a loss."""
    bounds = ASSERTED[name, filtered]
    cells = [_cells(name, spp, filtered) for spp in SPPS]
    print("%-6s %-8s %s" % (name, "filtered" if filtered else "raw", "   ".join("%3d spp %.4f -> %.4f" % (spp, a, b) for spp, (a, b) in zip(SPPS, cells))))
    for spp, (raw, res), bound in zip(SPPS, cells, bounds):
        assert np.isfinite(raw) and np.isfinite(res)
        if bound is not None:
            assert res <= bound * raw, (name, filtered, spp, raw, res, bound)


def test_the_partially_covered_pixels_of_c3_with_the_sky_shown():
    """Restricted to the 446 pixels with 0.02 < kappa < 0.98, where the coin toss is: 0.3951 -> 0.1415 at 2 spp, 0.0748 -> 0.0360 at 64 spp (measured);
    asserted at the whole frame's margin, resolved <= 0.75 x raw"""
    ref, guide = _reference("c3env"), _guide("c3env")
    m = (guide[..., 3] > 0.02) & (guide[..., 3] < 0.98)
    assert m.sum() > 100
    for spp in (2, 64):
        fb, _ = _inputs("c3env", spp)
        y, _ = hr.resolved(_oracle("c3env"), RAYS, fb, guide)
        raw, res = scenes.rel_l2(fb[..., :3][m], ref[m]), scenes.rel_l2(y[..., :3][m], ref[m])
        print("c3env, %d pixels with 0.02 < kappa < 0.98, %d spp: %.4f -> %.4f" % (int(m.sum()), spp, raw, res))
        assert res <= 0.75 * raw


# ---- 4: bias -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c2", "c3env"))
def test_the_bias_at_1024_spp_is_recorded(name):
    """Raw and resolved frames of seed 42 against 4096 spp of seed 1234567, 64x48, relative L2 of RGB.  Nothing is asserted but that the run is finite.
    Measured (frame -> resolved; then the mean of alpha - kappa and of its absolute value over the frame):
      c2     256 spp   0.02522 -> 0.02457    +0.00041   0.00301
      c2    1024 spp   0.01394 -> 0.01427    +0.00039   0.00193
      c3env  256 spp   0.01385 -> 0.00909    +0.00013   0.00303
      c3env 1024 spp   0.00655 -> 0.00613    +0.00008   0.00182
    Without a LUT (c2) the tracker's coverage lies 0.0004 above the march's on average; beta times that stays in y.  At 1024 spp the resolved frame is
    2.4 % worse than the raw one: with a fifth of either squared error being the reference's own noise and the variance ratio of the 64-spp cell
    ((0.0523 / 0.0530)^2), the bias comes to about 0.0036 relative L2, which the variance saved (0.026 sigma^2 / n) outweighs up to about 300 spp --
    it still pays at 256 spp (2.6 %).  Under the LUT (c3env) tracker and march agree, and the call pays at every count measured."""
    ref = _oracle(name, seed=1234567).render(4096).copy()[..., :3]
    guide = _guide(name)
    for spp in (256, 1024):
        fb = _frame(name, spp)
        y, _ = hr.resolved(_oracle(name), RAYS, fb, guide)
        raw, res = scenes.rel_l2(fb[..., :3], ref), scenes.rel_l2(y[..., :3], ref)
        dk = fb[..., 3].astype(np.float64) - guide[..., 3]
        print("%s at %d spp against 4096 spp: raw %.5f resolved %.5f   mean (alpha - kappa) %.5f, mean |alpha - kappa| %.5f" %
              (name, spp, raw, res, float(dk.mean()), float(np.abs(dk).mean())))
        assert np.isfinite(raw) and np.isfinite(res)
