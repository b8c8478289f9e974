"""CPU: the conservation laws of the path tracer's work counts, host lane code against the oracle.

The host build of the lane code (tests/hostkernel/host_kernel.cpp), walking exactly the items the device walks for a tile list, counts its lane steps by the state
they were entered in and the transitions that end a path or an item; the oracle counts the reference's events (orc_counters).  For the scene of each of the 14
compiled forms, on every frame and call split of tests/sched_cases.py, per call:

  1. new - outside == samples                    every item inside the frame starts one path, every other item starts none
  2. nee == postnee == n_nee                     a real collision is one NEE event and, after its shadow segment or at once, one scatter event
  3. ended == n_ended                            POSTNEE -> NEW: a path ended by the bounce cap or the roulette (free_path == 0)
  4. escape == samples - ended                   a path ends once: by an ESCAPE event or in the scatter event; == n_esc where the environment is shown (the
                                                 reference fetches it only then), and n_esc == 0 where it is not -- the law holds all the same
  5. primary_miss == n_primary_miss              NEW -> ESCAPE on a camera ray that misses the box.  With the DDA trackers that is every NEW -> ESCAPE; the
                                                 global-majorant trackers also go there from a ray that hits the box and draws its first free flight beyond it
                                                 (begin_segment), which the reference counts nowhere: new_escape >= primary_miss for them
  6. collide == n_coll_sv + n_coll_tr            one COLLIDE step is one evaluation of the reference's collision density.  collide_finish's shortcut for a blocked
                                                 shadow ray replaces the tail of that ONE step (the division and a roulette whose outcome is fixed): no step
                                                 fewer, so the law is an equality for every form, the global-majorant trackers (which stay in COLLIDE) included
  7. MARCH against n_dda_sv + n_dda_tr           NOT an equality: a march pass replays up to two iterations of the reference's DDA loop (the second prepared
                                                 speculatively), and a pass entered with t >= far -- a segment shorter than its 1e-6 offset, or one whose second
                                                 iteration stepped out of the box without a tentative collision -- replays none: the reference's `while` fails there.
                                                 What holds: march_dda == n_dda exactly, where march_dda is the iterations the passes went through, read off
                                                 march_prep / march_load with march_finish's own tests; and so, with march_empty the passes that went through none,
                                                 march - march_empty <= n_dda <= 2 (march - march_empty).  The global-majorant trackers never march: 0 == 0.

Found with these laws: the oracle's n_primary_miss stayed 0 under the global-majorant trackers (sample_volume_global did not report the box test to trace_path).
tests/test_gpu_sched_counts.py holds the device's instrumented instances to the same host counts."""
import numpy as np
import pytest

import hk_binding as hk
from hk_common import same as _same
import sched_cases as sc
from test_host_kernel import FORM_SCENES

CELLS = [(form, frame) for form in hk.FORMS for frame in sc.FRAMES]
_ids = lambda v: sc.form_id(v) if isinstance(v, tuple) else v


def _laws(form, frame, n, h, o):
    """one call of n samples: host counters h, oracle counters o"""
    _, o_scene = sc.oracle_scene(form, frame)
    global_trackers = FORM_SCENES[form][2] != 0
    samples = sc.pixels_of(frame) * n
    what = (sc.form_id(form), frame, n, h, o)
    assert o["samples"] == samples, what
    assert h["new"] == len(sc.tiles_of(frame)) * 256 * n, what                   # the device's items: 256 per listed tile and sample
    assert h["new"] - h["outside"] == samples, what                              # 1
    assert h["nee"] == h["postnee"] == o["n_nee"], what                          # 2
    assert h["ended"] == o["n_ended"], what                                      # 3
    assert h["escape"] == samples - h["ended"], what                             # 4
    if o_scene.show_environment:
        assert h["escape"] == o["n_esc"], what
    else:
        assert o["n_esc"] == 0, what
    assert h["primary_miss"] == o["n_primary_miss"], what                        # 5
    if global_trackers:
        assert h["new_escape"] >= h["primary_miss"], what
    else:
        assert h["new_escape"] == h["primary_miss"], what
    assert h["collide"] == o["n_coll_sv"] + o["n_coll_tr"], what                 # 6
    n_dda = o["n_dda_sv"] + o["n_dda_tr"]                                        # 7
    assert h["march_dda"] == n_dda, what
    ran = h["march"] - h["march_empty"]
    assert ran <= n_dda <= 2 * ran, what
    if global_trackers:
        assert h["march"] == 0 and n_dda == 0, what
    # the harness's older counters say the same in their own split (clean / general segments), and nothing is counted twice
    assert h["clean_march"] + h["general_march"] == h["march"] and h["clean_collide"] + h["general_collide"] == h["collide"], what
    assert h["steps"] == h["new"] + h["march"] + h["collide"] + h["nee"] + h["postnee"] + h["escape"] + 64 * _units(form, frame, n), what
    assert h["shadow_segments"] <= h["nee"], what


def _units(form, frame, n):
    """work units of a call (each ends with one NEW -> DONE step per lane of the harness, counted in `steps` only)"""
    spu = min(n, 4 if form[0] in (1, 2, 4) else 8)                               # vr_variant.h pathtrace_unit_samples
    return len(sc.tiles_of(frame)) * 4 * ((n + spu - 1) // spu)


@pytest.mark.parametrize("frame", list(sc.FRAMES))
@pytest.mark.parametrize("form", hk.FORMS, ids=_ids)
def test_host_counts_obey_the_laws_against_the_oracle(form, frame):
    totals = {}
    for split, ns in sc.SPLITS.items():
        host, fb = sc.host_counts(form, frame, split)
        orc, want = sc.oracle_counts(form, frame, split)
        assert _same(fb, want), (sc.form_id(form), frame, split)                 # the tile walk renders the oracle's frame (zeros outside a tile list)
        for n, h, o in zip(ns, host, orc):
            _laws(form, frame, n, h, o)
        totals[split] = sc.host_total(form, frame, split)
    # samples are independent: 6 + 5 in two calls count what 11 in one call count (`steps` apart, which holds the harness's own NEW -> DONE steps, 64 per unit)
    for t in totals.values():
        del t["steps"]
    assert totals["6+5"] == totals["11"], (sc.form_id(form), frame)


@pytest.mark.parametrize("form", hk.FORMS, ids=_ids)
def test_no_law_is_vacuous(form):
    """From the host counts alone, on the ragged frame: every scene shows a path ended by the cap or the roulette, a primary miss, a shadow segment and an item outside
    the frame -- and marches and collides, so that no law compares zeros (the global-majorant trackers apart, which never march)."""
    h = sc.host_total(form, sc.RAGGED, "11")
    assert h["ended"] > 0 and h["primary_miss"] > 0 and h["shadow_segments"] > 0 and h["outside"] > 0, (sc.form_id(form), h)
    assert h["escape"] > h["new_escape"] and h["collide"] > 0 and h["nee"] > 0, (sc.form_id(form), h)
    if FORM_SCENES[form][2] == 0:
        assert h["march"] > 0 and 0 < h["march_dda"] < 2 * h["march"], (sc.form_id(form), h)      # passes of one iteration and of two both occur


def test_one_row_does_not_show_the_environment():
    """Law 4's second half: a scene with a transfer function hides the environment (n_esc stays 0), one without shows it"""
    shown = {sc.oracle_scene(f, sc.RAGGED)[1].show_environment for f in hk.FORMS}
    assert shown == {True, False}
