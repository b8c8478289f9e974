"""GPU: the device build of the deterministic math layer (vr_math.h) against the CPU oracle (oracle_math.h), bit for bit, over whole domains.

Every unary function is swept over all 2^32 bit patterns in chunks of 2^26: the device forms x from the bit pattern and returns only the results
(vr_math_sweep), the oracle compares a chunk in place on its OpenMP threads while the device computes the next one.  A mismatch ends the test
with the oracle's first eight examples; nothing is swept after it.  Two-operand and integer functions go through the array probe on the specials
cross product and on their live domains (tests/hk_math.py array_cases, the sets the CPU module test_math_host.py runs through the host build).
The tolerance-mode forms (VR_FAST_MATH) are measured against float64 and held to twice the recorded figure."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hk_math as hm

pytestmark = pytest.mark.gpu

CHUNK = 1 << 26
_bufs = []


def _buffers():
    if not _bufs:
        _bufs.extend(np.empty(CHUNK, np.float32) for _ in range(2))
    return _bufs


def _sweep(fn, first=0, total=1 << 32, b=0.0, judge=None):
    """Device results for bits(first + i), i < total, chunk by chunk, each handed to judge(start, count, results) -- by default the oracle's comparison, whose
    first mismatch fails the test.  One worker thread makes every device call; the judging overlaps the next chunk's launch and download."""
    import volren_amd
    from oracle import binding as ob
    bufs = _buffers()
    starts = list(range(first, first + total, CHUNK))

    def device(k):
        n = min(CHUNK, first + total - starts[k])
        return n, volren_amd.math_sweep(fn, starts[k], n, b, bufs[k & 1])

    def oracle(start, n, got):
        bad = ob.math_sweep_compare(fn, start, n, got, b)
        if bad:
            pytest.fail("sweep of fn %d, chunk at 0x%08x: %s" % (fn, start & 0xFFFFFFFF, bad))

    judge = judge or oracle
    t0 = time.time()
    with ThreadPoolExecutor(1) as ex:                    # leaving the block waits for the chunk in flight; after a failure no further one is started
        fut = ex.submit(device, 0)
        for k in range(len(starts)):
            n, got = fut.result()
            fut = ex.submit(device, k + 1) if k + 1 < len(starts) else None
            judge(starts[k], n, got)
    print("fn %d: %d bit patterns from 0x%08x in %.1f s" % (fn, total, first, time.time() - t0))


UNARY = [(hm.EXP, 0.0, "exp_"), (hm.LOG, 0.0, "log_"), (hm.SINCOS_S, 0.0, "sincos_.s"), (hm.SINCOS_C, 0.0, "sincos_.c"), (hm.ACOS, 0.0, "acos_"),
         (hm.ASIN, 0.0, "asin_"), (hm.ATAN2, 1.0, "atan_"), (hm.SIN, 0.0, "sin_"), (hm.COS, 0.0, "cos_"), (hm.TAN, 0.0, "tan_"),
         (hm.SANITIZE, 0.0, "sanitize"), (hm.FLOOR2I, 0.0, "floor2i"), (hm.HALF_RNE, 0.0, "float_to_half_rne"),
         (hm.HALF_DOWN, 0.0, "float_to_half_down"), (hm.HALF_UP, 0.0, "float_to_half_up"), (hm.RCP_EXACT, 0.0, "rcp_exact")]


@pytest.mark.parametrize("fn,b", [u[:2] for u in UNARY], ids=[u[2] for u in UNARY])
def test_sweep_all_bit_patterns(fn, b):
    """All 2^32 arguments.  atan_ is atan2_(x, 1): x / 1 is exact and x = 1 takes no quadrant correction.  rcp_exact against the oracle's 1.0f / x is the
    comparison tests/tools_rcp_exact.hip makes on the device alone."""
    _sweep(fn, b=b)


def test_sweep_log_unit_over_its_domain():
    """log_unit_ on every normal x in (0, 1] (0x00800000 .. 0x3F800000) against the oracle's log"""
    _sweep(hm.LOG_UNIT, first=0x00800000, total=0x3F800000 - 0x00800000 + 1)


def test_sweep_entry_point_rejects_what_it_cannot_run():
    import volren_amd
    with pytest.raises(volren_amd.VolrenError):
        volren_amd.math_sweep(hm.EXP, 0, (1 << 26) + 1, 0.0, np.empty((1 << 26) + 1, np.float32))
    for fn in (17, hm.UNORM8 + 1, 99, 104, -1):
        with pytest.raises(volren_amd.VolrenError):
            volren_amd.math_sweep(fn, 0, 16)
    got = volren_amd.math_sweep(hm.SANITIZE, 0xFFFFFFF8, 16)                  # first + i wraps
    assert np.array_equal(hm.bits(got), hm.sweep(hm.SANITIZE, 0xFFFFFFF8, 16))


@pytest.mark.parametrize("k", range(hm.N_ARRAY_CASES))
def test_array_cases_match_oracle(k):
    """specials cross products, live domains, integer helpers (voxel_index by the property its header states): device against oracle"""
    import volren_amd
    from oracle import binding as ob
    name, fn, a, b = hm.array_cases()[k]
    got = volren_amd.math_probe(fn, hm.f32(a), hm.f32(b) if b is not None else None)
    bad = ob.math_compare(fn, a, b, got)
    assert not bad, "%s (%d inputs): %s" % (name, a.size, bad)


def test_comparison_reports_a_one_bit_change():
    """the oracle's comparison sees a single flipped result bit, in a float and in an integer result, and does not let a NaN pass for an integer"""
    import volren_amd
    from oracle import binding as ob
    for fn in (hm.EXP, hm.FLOOR2I):
        got = hm.bits(volren_amd.math_sweep(fn, 0x3F000000, 4096).copy())
        assert not ob.math_sweep_compare(fn, 0x3F000000, 4096, got)
        got[1234] ^= 1
        bad = ob.math_sweep_compare(fn, 0x3F000000, 4096, got)
        assert bad.count == 1 and bad.examples[0][0] == 0x3F000000 + 1234


def test_specification_pins():
    """the conventions that differ from C's libm, as bit patterns: device, host build and oracle alike"""
    import volren_amd
    from oracle import binding as ob
    for what, fn, a, b, want in hm.SPEC_PINS:
        ab, bb = hm.bits(np.float32(a)), hm.bits(np.float32(b))
        for who, got in (("device", hm.bits(volren_amd.math_probe(fn, hm.f32(ab), hm.f32(bb)))), ("host build", hm.batch(fn, ab, bb)), ("oracle", ob.math_batch(fn, ab, bb))):
            assert hm.pin_holds(int(got[0]), want), "%s on the %s: got 0x%08x, want %s" % (what, who, got[0], "NaN" if want is None else "0x%08x" % want)


def _merge(parts):
    return {"max_ulp": max(p["max_ulp"] for p in parts), "max_abs": max(p["max_abs"] for p in parts), "points": sum(p["points"] for p in parts)}


def test_tolerance_mode_forms_against_float64():
    """The VR_FAST_MATH forms as functions (vr_fastprobe.hip, built with the tolerance-mode flags) against float64 over their live domains: neg_log_1m on every
    draw, sincos_ on [0, 2 pi] (which holds the [0, pi] of the polar angles), unorm8 on 0..255.  Held to twice the figures (absolute error; ulps too where the result has no zero inside the domain) recorded in
    tests/golden/math_accuracy.json: the hardware units are deterministic but contraction may move with the toolchain; a wrong constant or a dropped
    conversion to revolutions is orders of magnitude away."""
    import volren_amd
    got = {}
    dev = volren_amd.math_sweep(hm.FAST_NEG_LOG_1M, 0, 1 << 24).copy()
    got["neg_log_1m"] = _merge([hm.accuracy(hm.NEG_LOG_1M, hm.draws(), got=dev)])
    two_pi = int(hm.bits(np.float32(2.0 * np.pi))[0])
    for name, code, ref in (("sincos_.s", hm.FAST_SIN, hm.SINCOS_S), ("sincos_.c", hm.FAST_COS, hm.SINCOS_C)):
        parts = []
        _sweep(code, first=0, total=two_pi + 1, judge=lambda start, n, res: parts.append(hm.accuracy_sweep(ref, start, n, got=res)))
        got[name] = _merge(parts)
    dev = volren_amd.math_sweep(hm.FAST_UNORM8, 0, 256).astype(np.float64)
    want = np.arange(256, dtype=np.float64) / 255.0
    err = np.abs(dev - want)
    got["unorm8"] = {"max_ulp": float((err / np.maximum(np.spacing(want.astype(np.float32)).astype(np.float64), 2.0 ** -149)).max()), "max_abs": float(err.max()), "points": 256}
    for name in sorted(got):
        print("tolerance-mode %s: max %.4f ulp, max abs %.6e over %d points" % (name, got[name]["max_ulp"], got[name]["max_abs"], got[name]["points"]))
    rec = hm.recorded()["fast"]
    assert rec, "tests/golden/math_accuracy.json has no measured figures for the tolerance-mode forms"
    for name in sorted(got):
        assert got[name]["max_abs"] <= 2.0 * rec[name]["max_abs"], (name, got[name], rec[name])
        if not name.startswith("sincos_"):               # v_sin_f32 / v_cos_f32 are accurate in absolute terms: at a zero of the function the error in ulps has no bound worth holding
            assert got[name]["max_ulp"] <= 2.0 * rec[name]["max_ulp"], (name, got[name], rec[name])
