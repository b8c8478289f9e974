"""CPU: the walk of tests/walk_cases.py held to itself, with the oracle and the host builds alone.  tests/test_gpu_walk.py compares a walked renderer with
walk_cases.references after every step; that says something only if a step MOVES the read-backs it names (else a cache that ignored the step would pass), if a
step back really returns (else a cache stuck on the middle state would pass), if the walk visits the states its steps are there for, and if the classes it
expects are sound on the walk's own views."""
import numpy as np
import pytest

import hk_see_through as st
import walk_cases as wc
from hk_common import same

WALK = wc.states()
IDS = ["%02d-%s" % (i, w[0].replace(" ", "_")) for i, w in enumerate(WALK)]


def _equal(k, a, b):
    if k == "classes":
        return a == b
    return a.shape == b.shape and (np.array_equal(a, b) if a.dtype == np.uint8 else same(a, b))


def test_the_start_is_c2_at_72x56_with_its_pinned_classes():
    """tests/test_see_through_host.py pins 4 clear tiles and 1 see-through tile there; env_rot = 0 and the camera the state spells out are the configuration's own"""
    import scenes
    assert wc.tile_classes(wc.START) == (4, 1)
    o = scenes.oracle_scene("c2", 72, 56)
    a, b = wc.build_oracle(wc.START).params(), o.params()                # (but for the sign of one zero of the rotation by 0 degrees)
    assert all(np.array_equal(np.array(getattr(a, f)), np.array(getattr(b, f))) for f, _ in a._fields_)
    assert same(wc.references(wc.START)["frame"], o.render(wc.SPP))


def test_the_list_is_what_the_issue_lists():
    assert 35 <= len(wc.STEPS) and len(set(w[0] for w in WALK)) == len(WALK)
    assert WALK[-1][5] == wc.START                                     # the walk ends where it began
    straddled = set(k for w in WALK if w[3] for k in w[1])
    assert straddled == {"cam_pos", "cam_dir", "cam_fov", "vol_clip_min", "vol_clip_max", "seed", "show_environment", "env_rot", "integrator", "grid_frame_counter",
                         "sky_tiles", "see_through_tiles", "order_tiles", "seed_table_mb"}
    for name, change, targets, straddle, before, after in WALK:
        assert any(before[k] != after[k] for k in change), name        # a step changes something
        if straddle:                                                   # integrators 2 and 3 are other kernels, and never under the tolerance mode
            assert {before["integrator"], after["integrator"]} <= {0, 1} and not before["fast_math"] and not after["fast_math"], name
    i = [w[0] for w in WALK].index("fast_math 1")
    assert WALK[i + 1][0] == "fast_math 0"                             # nothing is compared under the tolerance mode but the step back


@pytest.mark.parametrize("i", range(len(WALK)), ids=IDS)
def test_no_step_is_vacuous(i):
    """every read-back a step names differs, in the references, from what it was before the step"""
    name, change, targets, straddle, before, after = WALK[i]
    a, b = wc.references(before), wc.references(after)
    still = sorted(k for k in targets if _equal(k, a[k], b[k]))
    assert not still, "'%s' does not move %s" % (name, still)


def test_every_step_back_is_a_real_return():
    """the walk ends where it began (test_the_list_is_what_the_issue_lists), so every field is taken back; where a step lands on a state the walk has been in,
    the references computed again from nothing are those of the first visit, bit for bit"""
    seen, returns = {wc.key(wc.START): wc.references(wc.START)}, 0
    for i, (name, change, targets, straddle, before, after) in enumerate(WALK):
        k = wc.key(after)
        if k in seen:
            again = wc.references(after, fresh=True)
            for rb in wc.READ_BACKS:
                assert _equal(rb, again[rb], seen[k][rb]), (name, rb)
            returns += 1
        else:
            seen[k] = wc.references(after)
    assert returns >= 10                                              # (whole states, switches included: the scene alone comes back more often)


def _visit(pred):
    return [w[5] for w in WALK if pred(w[5])]


def test_the_walk_reaches_what_it_claims():
    cls = {wc.key(w[5]): wc.tile_classes(w[5]) for w in WALK}
    n_tiles = {wc.key(w[5]): len(wc.tile_ids(w[5])) for w in WALK}
    assert any(c > 0 and s > 0 for c, s in cls.values())
    assert any(c == n_tiles[k] for k, (c, s) in cls.items())                                          # every tile clear: no path-tracing launch
    inside = _visit(lambda s: s["cam_pos"] == (0.02, 0.01, 0.03))
    assert inside and all(wc.tile_classes(dict(s, see_through_tiles=1, sky_tiles=1)) == (0, 0) for s in inside)      # none clear
    assert cls[wc.key([w[5] for w in WALK if w[0] == "resize 128x128"][0])] == (16, 7)
    lut = _visit(lambda s: s["lut"] is not None and s["integrator"] == 0)
    assert lut and all(wc.tile_classes(s)[1] == 0 and wc.tile_classes(s)[0] > 0 for s in lut)          # the see-through class goes to 0 behind a LUT, the clear one stays
    assert _visit(lambda s: s["temperature"] is not None)
    assert _visit(lambda s: s["density_scale"] == 2.0 ** -17) and _visit(lambda s: s["integrator"] == 2 and s["lut"] is not None) and _visit(lambda s: s["integrator"] == 3)
    anim = _visit(lambda s: s["volume"] != "smoke")
    f0, f1 = [s for s in anim if s["grid_frame_counter"] == 0][0], [s for s in anim if s["grid_frame_counter"] == 1][0]
    for t in ("table1", "table2"):
        a, b = wc.references(f0)[t], wc.references(f1)[t]
        assert a.shape == b.shape and not np.array_equal(a, b) and (a == 0).any() and (a > 0).any()
    assert not np.array_equal(wc.references(wc.START)["table1"], wc.references(wc.START)["table2"])      # the two reaches are two tables
    a, b = ([w[5] for w in WALK if w[0].startswith(n)][0] for n in ("tile subset A", "tile subset B"))
    assert len(a["tiles"]) == len(b["tiles"]) and wc.tile_classes(a) != wc.tile_classes(b)
    assert wc.tile_classes(b)[1] == 1 and wc.tile_classes(b)[0] > 0


@pytest.mark.parametrize("which", ["camera turned about the volume", "clip box x in [0.25, 0.75]", "frame 1 replaced and committed", "brick frame 1"])
def test_the_reference_stays_sound_over_the_walk(which):
    """tests/test_see_through_host.py's soundness check on the walk's own views: no ray of the quarter-pixel lattice over a see-through tile comes within tap reach
    of a live brick.  (The animation's float frames are encoded on the device, so the product has no see-through tile there; the classifier is asked what it would
    say if the host held the table -- which is what a stale list made for another grid would be judged against.)"""
    state = [w[5] for w in WALK if w[0] == which][0]
    state = dict(state, see_through_tiles=1)
    o = wc.build_oracle(state)
    cls, _ = st.classify(o, wc.tile_ids(state))
    see, march = np.flatnonzero(cls == st.SEE), np.flatnonzero(cls == st.MARCH)
    assert see.size > 0 and march.size > 0
    assert not st.lattice_touches(o, see).any()
    assert st.lattice_touches(o, march[:4]).any()
