"""CPU: collide_finish (vr_trace.h) built for the host in both of its orders -- the reference's, and the one that evaluates what the path's state alone
determines (both LCG advances, the second draw, its neg_log_1m, the shortcut's premises) before the tap's value is used and commits the outcome afterwards.

Every field of Hot the function may touch -- state, seed, tau, t, Tr, mipq, majorant -- and the collision colour a transfer-function kernel leaves on the cold
line, bit for bit: the two orders against each other, and both against the reference's expressions (transmittanceDDA's as written out in
test_collide_shadow_host.py, sample_volumeDDA's here).  Camera and shadow segments; real and null collisions; a draw of exactly 0 and the largest draw, first and
second; the shortcut's edges (cell majorant one ulp below, equal to and one ulp above vol_majorant, zero, negative, infinite, NaN; a NaN vol_majorant; an
overflowed Tr); each with and without a transfer function."""
import itertools

import numpy as np
import pytest

import hk_collide_tail
import hk_math
from test_collide_shadow_host import DENSITIES, MAJORANTS, SEEDS, TRS, bits, draw, reference

F = np.float32
ST_MARCH, ST_NEE, ST_POSTNEE = 2, 4, 5
TAU_IN, T_IN = 0.8125, 17.25                    # what a field holds before the call: a collision that does not write it leaves this
MIPQS = (12, 5)                                 # mip = max(0, mip - 2) in quarter steps: 4, and clamped to 0
LUT_RGB = (0.25, 0.5, 0.75)


def _cases():
    return list(itertools.product(SEEDS, MAJORANTS, TRS, DENSITIES, (0, 1), MIPQS))


def _states(cases):
    return np.array([[s, bits(m), bits(vm), bits(tr), bits(d), shadow, mipq, bits(TAU_IN), bits(T_IN)] for s, (m, vm), tr, d, shadow, mipq in cases], np.uint32)


def _density(tf, vm, d):
    """the density the collision tests: the tap's value, or -- transfer function -- vol_majorant * alpha"""
    with np.errstate(all="ignore"):
        return F(vm) * F(d) if tf else F(d)


def camera_reference(seed, majorant, d):
    """sample_volumeDDA from its test of a tentative collision to the next free-flight draw: (state, seed, draw behind tau or None)"""
    with np.errstate(all="ignore"):
        seed, r = draw(seed)
        if r * F(majorant) < F(d):
            return ST_NEE, seed, None
        seed, r = draw(seed)
    return ST_MARCH, seed, r


def _is_nan(b):
    return (int(b) & 0x7FFFFFFF) > 0x7F800000


def test_the_shared_states_hold_the_edges_this_file_names():
    assert any(np.isnan(vm) for _, vm in MAJORANTS) and any(np.isnan(m) for m, _ in MAJORANTS) and any(np.isinf(t) for t in TRS)
    assert {m for m, vm in MAJORANTS if vm == 3.0} >= {float(np.nextafter(F(3.0), F(0))), 3.0, float(np.nextafter(F(3.0), F(np.inf))), 0.0, -1.5, float("inf")}


@pytest.mark.parametrize("tf", (0, 1), ids=("no_tf", "tf"))
def test_both_orders_leave_the_same_path(tf):
    st = _states(_cases())
    a, b = hk_collide_tail.collide(tf, 0, st), hk_collide_tail.collide(tf, 1, st)
    # a NaN Tr (inf x 0) is a NaN in both; everything else is the same word
    nan = np.array([_is_nan(x) for x in a[:, 4]])
    assert np.array_equal(nan, np.array([_is_nan(x) for x in b[:, 4]]))
    keep = np.ones(a.shape[1], bool)
    keep[4] = False
    assert np.array_equal(a[~nan], b[~nan])
    assert np.array_equal(a[nan][:, keep], b[nan][:, keep])


@pytest.mark.parametrize("early", (0, 1), ids=("reference_order", "early_tail"))
@pytest.mark.parametrize("tf", (0, 1), ids=("no_tf", "tf"))
def test_each_order_matches_the_reference_expression(tf, early):
    cases = _cases()
    got = hk_collide_tail.collide(tf, early, _states(cases))
    tau_draws, tau_rows = [], []
    ends = {ST_MARCH: 0, ST_NEE: 0, ST_POSTNEE: 0}
    fell_back = 0
    for i, (s, (m, vm), tr, d, shadow, mipq) in enumerate(cases):
        dens = _density(tf, vm, d)
        what = "seed %#x majorant %r vol_majorant %r Tr %r density %r shadow %d mipq %d" % (s, m, vm, tr, d, shadow, mipq)
        if shadow:
            Tr, state, seed, r = reference(s, m, vm, tr, dens)
            if state == ST_POSTNEE and not (0.0 < m <= vm and abs(tr) < float("inf")):
                fell_back += 1
        else:
            state, seed, r = camera_reference(s, m, dens)
            Tr = F(tr)
        ends[state] += 1
        assert int(got[i, 0]) == state, what
        assert int(got[i, 1]) == seed, what
        assert int(got[i, 3]) == bits(T_IN), what
        if np.isnan(Tr):
            assert _is_nan(got[i, 4]), what
        else:
            assert int(got[i, 4]) == bits(Tr), what
        assert int(got[i, 6]) == bits(m), what
        if state == ST_MARCH:
            tau_draws.append(r)
            tau_rows.append(i)
            assert int(got[i, 5]) == max(0, mipq - 8), what
        else:
            assert int(got[i, 2]) == bits(TAU_IN) and int(got[i, 5]) == mipq, what
        colour = [bits(x) for x in LUT_RGB] if (tf and state == ST_NEE) else [bits(-1.0)] * 3
        assert [int(x) for x in got[i, 7:10]] == colour, what
    want_tau = hk_math.batch(hk_math.NEG_LOG_1M, np.array(tau_draws, np.float32))
    assert np.array_equal(got[tau_rows, 2], want_tau)                  # (uint32 result bits on both sides)
    # the cases reach every end: a null collision, a real one on both kinds of segment, the shortcut's and the roulette behind it
    assert all(n > 0 for n in ends.values()) and ends[ST_POSTNEE] > fell_back > 0
