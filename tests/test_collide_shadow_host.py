"""CPU: a shadow ray at a tentative collision of the DDA trackers -- collide_finish (vr_trace.h) built for the host -- against the reference's expression
(common.glsl transmittanceDDA, :442-452) written out here, bit for bit.

Since round 7 a blocked shadow ray whose cell majorant does not exceed the volume's ends without the division and the roulette, whose outcome is fixed
there (the argument is at the shortcut).  Every scene the product builds has only such cells, so the frames the other tests render never reach the code
behind the shortcut: the states below do -- a majorant one ulp and far above vol_majorant, zero, negative, infinite, NaN, a NaN vol_majorant, an
overflowed Tr -- and the states on the shortcut's side of each edge sit beside them."""
import itertools

import numpy as np
import pytest

import hk_hotpair as hk_collide
import hk_math

F = np.float32
ST_MARCH, ST_POSTNEE = 2, 5
A, Cc, M32 = 1664525, 1013904223, 1 << 32
A_INV = pow(A, -1, M32)


def lcg(s):
    return (s * A + Cc) % M32


def draw(s):
    """rng(): the state after the advance and its draw"""
    s = lcg(s)
    return s, F(s & 0xFFFFFF) * F(1.0 / 16777216.0)


def state_before(low24, high8, draws_ahead):
    """an LCG state whose `draws_ahead`-th draw from here has the 24 bits `low24`"""
    s = (high8 << 24) | low24
    for _ in range(draws_ahead):
        s = ((s - Cc) * A_INV) % M32
    return s


def bits(x):
    return int(np.array(x, np.float32).view(np.uint32))


def reference(seed, majorant, vol_majorant, Tr, d):
    """transmittanceDDA from its test of a tentative collision to the next free-flight draw: (Tr, state, seed, draw behind tau or None)"""
    majorant, vol_majorant, Tr, d = F(majorant), F(vol_majorant), F(Tr), F(d)
    with np.errstate(all="ignore"):
        seed, r = draw(seed)
        if r * majorant < d:                                        # real collision
            x = F(1.0) - vol_majorant / majorant
            Tr = Tr * (x if F(0.0) < x else F(0.0))                 # max(0.f, .) as the product specifies it: the first argument unless 0 < x
            if Tr < F(0.1):
                prob = F(1.0) - Tr
                seed, r = draw(seed)
                if r < prob:
                    return F(0.0), ST_POSTNEE, seed, None
                Tr = Tr / (F(1.0) - prob)
        seed, r = draw(seed)
    return Tr, ST_MARCH, seed, r


NAN, INF = float("nan"), float("inf")
VOL = 3.0
UP = float(np.nextafter(F(VOL), F(INF)))
DOWN = float(np.nextafter(F(VOL), F(0)))
# (cell majorant, vol_majorant): below, one ulp below, equal, one ulp above, far above, NaN; then what only a broken table holds
MAJORANTS = [(1.5, VOL), (DOWN, VOL), (VOL, VOL), (UP, VOL), (300.0, VOL), (NAN, VOL),
             (0.0, VOL), (-0.0, VOL), (-1.5, VOL), (INF, VOL), (INF, INF), (1.5, INF), (1.5, NAN), (-3.0, -1.5), (1e-45, VOL), (0.0, 0.0)]
TRS = [1.0, 0.5, 0.05, 1e-30, 0.0, INF]
DENSITIES = [1e30, 1.0, 0.0]                                       # always a real collision; one by the draw; never
# RNG states: the first / the second draw from here is 0 or (2^24 - 1) / 2^24, and two ordinary ones
SEEDS = [state_before(0, 0x5A, 1), state_before(0xFFFFFF, 0xA5, 1), state_before(0, 0x33, 2), state_before(0xFFFFFF, 0xCC, 2), 42, 0xDEADBEEF]


def _cases():
    return list(itertools.product(SEEDS, MAJORANTS, TRS, DENSITIES))


def _states(cases):
    return np.array([[s, bits(m), bits(vm), bits(tr), bits(d)] for s, (m, vm), tr, d in cases], np.uint32)


def test_crafted_seeds_draw_what_they_should():
    for s, n, want in ((SEEDS[0], 1, 0.0), (SEEDS[1], 1, 16777215.0 / 16777216.0), (SEEDS[2], 2, 0.0), (SEEDS[3], 2, 16777215.0 / 16777216.0)):
        for _ in range(n):
            s, r = draw(s)
        assert r == F(want)
    assert F(16777215.0 / 16777216.0) < F(1.0)


@pytest.mark.parametrize("shortcut", (True, False), ids=("shortcut", "reference_tail_only"))
@pytest.mark.parametrize("form", (0, 1), ids=("one_scene_kind", "run_time"))
def test_shadow_collision_matches_the_reference_expression(form, shortcut):
    cases = _cases()
    got = hk_collide.shadow_collide(form, _states(cases), shortcut=shortcut)
    tau_draws, tau_rows = [], []
    terminated = fell_back = 0
    for i, (s, (m, vm), tr, d) in enumerate(cases):
        Tr, state, seed, r = reference(s, m, vm, tr, d)
        what = "seed %#x majorant %r vol_majorant %r Tr %r density %r" % (s, m, vm, tr, d)
        assert int(got[i, 1]) == state, what
        assert int(got[i, 2]) == seed, what
        if np.isnan(Tr):
            assert (int(got[i, 0]) & 0x7FFFFFFF) > 0x7F800000, what
        else:
            assert int(got[i, 0]) == bits(Tr), what
        if state == ST_POSTNEE:
            terminated += 1
            if not (0.0 < m <= vm and abs(tr) < INF):
                fell_back += 1
        else:
            tau_draws.append(r)
            tau_rows.append(i)
            assert int(got[i, 4]) == 4, what                       # mip = max(0, mip - 2) from 3, in quarter steps
    # tau = -log(1 - draw): the math layer's own function (held to the oracle by the math tests)
    want_tau = hk_math.batch(hk_math.NEG_LOG_1M, np.array(tau_draws, np.float32))
    assert np.array_equal(got[tau_rows, 3], want_tau)
    # the cases do reach all three ends: the shortcut's, the roulette behind it, and the march going on
    assert terminated > fell_back > 0 and len(tau_rows) > 0


def test_both_builds_agree_state_by_state():
    st = _states(_cases())
    for form in (0, 1):
        a, b = hk_collide.shadow_collide(form, st, True), hk_collide.shadow_collide(form, st, False)
        nan = (a[:, 0] & 0x7FFFFFFF) > 0x7F800000
        assert np.array_equal(nan, (b[:, 0] & 0x7FFFFFFF) > 0x7F800000)
        assert np.array_equal(a[~nan], b[~nan]) and np.array_equal(a[nan][:, 1:], b[nan][:, 1:])
