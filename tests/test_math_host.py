"""CPU: the host build of the deterministic math layer (vr_math.h behind vr_math_probe.h) against the CPU oracle (oracle_math.h), bit for bit, on a
lattice of every exponent x both signs x 2^14 mantissas, on the specials cross products and live domains the GPU module (test_gpu_math.py) runs on
the device, and over all 2^24 draws of neg_log_1m and all 2^16 halves.  The half encoders are held to properties (numpy's cast, bracketing), and the
accuracy against float64 libm to the maxima recorded in tests/golden/math_accuracy.json (measured exhaustively by tests/tools_math_accuracy.py)."""
import numpy as np
import pytest

import hk_math as hm
from oracle import binding as ob

LATTICE_FNS = [(hm.LOG, None, "log_"), (hm.SIN, None, "sin_"), (hm.COS, None, "cos_"), (hm.TAN, None, "tan_"), (hm.ACOS, None, "acos_"), (hm.ASIN, None, "asin_"),
               (hm.EXP, None, "exp_"), (hm.ATAN2, 1.0, "atan_"), (hm.SINCOS_S, None, "sincos_.s"), (hm.SINCOS_C, None, "sincos_.c"), (hm.SANITIZE, None, "sanitize"),
               (hm.FLOOR2I, None, "floor2i"), (hm.HALF_RNE, None, "float_to_half_rne"), (hm.HALF_DOWN, None, "float_to_half_down"),
               (hm.HALF_UP, None, "float_to_half_up"), (hm.RCP_EXACT, None, "rcp_exact"), (10, None, "sqrt_")]


@pytest.fixture(scope="module")
def lattice():
    u = hm.lattice(1 << 14)
    u.setflags(write=False)
    return u


@pytest.mark.parametrize("fn,b", [f[:2] for f in LATTICE_FNS], ids=[f[2] for f in LATTICE_FNS])
def test_host_matches_oracle_on_lattice(lattice, fn, b):
    bb = None if b is None else hm.bits(np.float32(b))
    bad = ob.math_compare(fn, lattice, bb, hm.batch(fn, lattice, bb))
    assert not bad, str(bad)


def test_log_unit_matches_oracle_on_its_domain(lattice):
    x = hm.f32(lattice)
    u = lattice[(x >= np.float32(1.17549435e-38)) & (x <= 1.0)]
    assert u.size > 1000000
    bad = ob.math_compare(hm.LOG_UNIT, u, None, hm.batch(hm.LOG_UNIT, u))
    assert not bad, str(bad)
    assert np.array_equal(hm.batch(hm.LOG_UNIT, u), hm.batch(hm.LOG, u))


@pytest.mark.parametrize("k", range(hm.N_ARRAY_CASES))
def test_host_array_cases_match_oracle(k):
    assert len(hm.array_cases()) == hm.N_ARRAY_CASES
    name, fn, a, b = hm.array_cases()[k]
    bad = ob.math_compare(fn, a, b, hm.batch(fn, a, b))
    assert not bad, "%s (%d inputs): %s" % (name, a.size, bad)


def test_sweep_form_equals_array_form():
    first = 0xFFFFFF00                                   # wraps through 0
    a = (np.arange(512, dtype=np.uint64) + first).astype(np.uint32)
    for fn, b in ((hm.EXP, 0.0), (hm.ATAN2, 1.0), (hm.HALF_UP, 0.0)):
        assert np.array_equal(hm.sweep(fn, first, 512, b), hm.batch(fn, a, hm.bits(np.float32(b))))
        assert not ob.math_sweep_compare(fn, first, 512, hm.sweep(fn, first, 512, b), b)


def test_comparison_reports_a_one_bit_change(lattice):
    """a single flipped bit in one result is counted and located, for a float and an integer result; NaN passes for NaN in float results only"""
    u = lattice[:200000]
    for fn in (hm.EXP, hm.MIN, hm.FLOOR2I, hm.HALF_RNE):
        got = hm.batch(fn, u, u)
        assert not ob.math_compare(fn, u, u, got)
        got[77777] ^= 1
        bad = ob.math_compare(fn, u, u, got)
        assert bad.count == 1 and bad.examples[0][0] == 77777 and bad.examples[0][1] == bad.examples[0][2] ^ 1
    nan = np.array([0x7FC00000], np.uint32)
    assert not ob.math_compare(hm.LOG, hm.bits(np.float32(-1.0)), None, nan ^ np.uint32(0x80000001))          # any NaN for the oracle's NaN
    assert ob.math_compare(hm.FLOOR2I, hm.bits(np.float32(1.0)), None, nan).count == 1
    got = hm.sweep(hm.EXP, 0x3F000000, 4096)
    got[5] ^= 1
    bad = ob.math_sweep_compare(hm.EXP, 0x3F000000, 4096, got)
    assert bad.count == 1 and bad.examples[0][0] == 0x3F000005
    with pytest.raises(ValueError):
        ob.math_compare(99, u, None, u)


def test_voxel_index_property_is_what_the_comparison_checks():
    """inside [0, 2^30) the index must be the host's; outside, anything negative or >= 2^30 passes and anything inside fails"""
    x = hm.bits(np.array([5.0, 5.0, 3e9, 3e9, -3e9, 2147483520.0], np.float32))
    o = np.array([2, 2, 1, 1, -2, 2], np.int32).view(np.uint32)
    got = np.array([7, 8, 0x80000001, 17, 0x7FFFFFFE, 0x80000001], np.uint32)
    bad = ob.math_compare(hm.VOXEL_INDEX, x, o, got)
    assert bad.count == 2 and [e[0] for e in bad.examples] == [1, 3]


def test_specification_pins():
    for what, fn, a, b, want in hm.SPEC_PINS:
        ab, bb = hm.bits(np.float32(a)), hm.bits(np.float32(b))
        for who, got in (("host build", hm.batch(fn, ab, bb)), ("oracle", ob.math_batch(fn, ab, bb))):
            assert hm.pin_holds(int(got[0]), want), "%s on the %s: got 0x%08x" % (what, who, got[0])


# ---- the half encoders, against properties ----------------------------------------------------------------------------------------------------
def _half_inputs(lattice):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = hm.bits(h.view(np.float16).astype(np.float32))
    f = f[~np.isnan(hm.f32(f))]
    return np.concatenate([lattice, f - 1, f, f + 1]).astype(np.uint32)


def test_half_rne_is_numpys_cast(lattice):
    u = _half_inputs(lattice)
    x = hm.f32(u)
    got = hm.batch(hm.HALF_RNE, u)
    assert (got >> 16 == 0).all()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).view(np.uint16).astype(np.uint32)
    nan = np.isnan(x)
    assert np.array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7FFF) > 0x7C00).all() and np.array_equal(got[nan] >> 15, u[nan] >> 31)          # a NaN stays a NaN of the same sign (the payload is not rounding)


def test_half_down_and_up_bracket_with_no_half_between(lattice):
    u = _half_inputs(lattice)
    u = u[np.isfinite(hm.f32(u))]
    x = hm.f32(u)
    d = hm.batch(hm.HALF_DOWN, u).astype(np.uint16).view(np.float16)
    p = hm.batch(hm.HALF_UP, u).astype(np.uint16).view(np.float16)
    df, pf = d.astype(np.float32), p.astype(np.float32)
    assert (df <= x).all() and (x <= pf).all()
    with np.errstate(over="ignore"):                                                   # the half after 65504 is inf
        assert (np.nextafter(d, np.float16(np.inf)).astype(np.float32) > x).all()      # the half after down(f) is already above f
        assert (np.nextafter(p, np.float16(-np.inf)).astype(np.float32) < x).all()     # the half before up(f) is already below f
    z = hm.bits(np.array([0.0, -0.0], np.float32))
    assert hm.batch(hm.HALF_DOWN, z).tolist() == [0, 0x8000] and hm.batch(hm.HALF_UP, z).tolist() == [0, 0x8000]
    inf = hm.bits(np.array([np.inf, -np.inf], np.float32))
    assert hm.batch(hm.HALF_DOWN, inf).tolist() == [0x7C00, 0xFC00] and hm.batch(hm.HALF_UP, inf).tolist() == [0x7C00, 0xFC00]


def test_half2float_is_numpys_cast():
    h = np.arange(65536, dtype=np.uint32)
    got = hm.batch(hm.HALF2FLOAT, h)
    want = hm.bits(h.astype(np.uint16).view(np.float16).astype(np.float32))
    nan = np.isnan(hm.f32(want))
    assert np.array_equal(got[~nan], want[~nan]) and np.isnan(hm.f32(got[nan])).all()


# ---- accuracy against float64 ----------------------------------------------------------------------------------------------------------------------
ACCURACY = [(hm.LOG, "log_"), (hm.SIN, "sin_"), (hm.COS, "cos_"), (hm.TAN, "tan_"), (hm.ACOS, "acos_"), (hm.ASIN, "asin_"), (hm.EXP, "exp_"),
            (hm.SINCOS_S, "sincos_.s"), (hm.SINCOS_C, "sincos_.c"), (hm.NEG_LOG_1M, "neg_log_1m"), (hm.ATAN2, "atan2_"), (hm.POW, "pow_"),
            (hm.SINCOS_S, "sincos_.s" + hm.LIVE), (hm.SINCOS_C, "sincos_.c" + hm.LIVE)]


@pytest.mark.parametrize("fn,name", ACCURACY, ids=[a[1] for a in ACCURACY])
def test_accuracy_against_float64(lattice, fn, name):
    """The oracle's results on the lattice (two-operand functions and neg_log_1m: on their live sets) against float64 libm, on the domain vr_math.h specifies,
    in ulps of the correctly rounded float32 result; sin and cos also in absolute terms (tan's absolute error is unbounded near its poles).  Each maximum
    is at most the recorded one -- exhaustive for the unary functions -- rounded up to the next 0.05: the functions are deterministic, the margin covers the
    float64 reference's own error and another host's libm."""
    rec = hm.recorded()["exact"][name]
    if fn == hm.NEG_LOG_1M:
        a, b = hm.draws(), None
    elif fn == hm.ATAN2:
        a, b = hm.unit_directions()
    elif fn == hm.POW:
        a, b = hm.pow_domains()
    elif name.endswith(hm.LIVE):
        a, b = np.concatenate([lattice[lattice <= hm.TWO_PI_BITS], np.linspace(0.0, 2.0 * np.pi, 1 << 20).astype(np.float32).view(np.uint32)]), None
    else:
        a, b = lattice, None
    r = hm.accuracy(fn, a, b, got=ob.math_batch(fn, a, b))
    print("%s: max %.4f ulp at %s (recorded %.4f), max abs %.4f x 2^-24, %d points in the domain" % (
        name, r["max_ulp"], ["0x%08x" % w for w in r["worst"]], rec["max_ulp"], r["max_abs"] * 2.0 ** 24, r["points"]))
    assert r["points"] > 100000
    assert r["max_ulp"] <= hm.bound(rec["max_ulp"])
    if "max_abs_2p-24" in rec:
        assert r["max_abs"] * 2.0 ** 24 <= hm.bound(rec["max_abs_2p-24"])


def test_accuracy_measure_sees_a_one_ulp_error():
    """the float64 comparison itself: one ulp added to every result moves the maximum by one ulp"""
    u = hm.bits(np.linspace(0.5, 2.0, 4097, dtype=np.float32))
    got = hm.batch(hm.LOG, u)
    base = hm.accuracy(hm.LOG, u, got=got)["max_ulp"]
    moved = hm.accuracy(hm.LOG, u, got=got + 1)["max_ulp"]
    assert base < 1.0 and 0.5 < moved - base or moved > 1.0
    assert hm.accuracy(hm.LOG, hm.bits(np.float32([-1.0, 0.0, np.inf, np.nan])))["points"] == 0         # outside the specified domain: not judged
