"""GPU: ONE live renderer walked through the committed list of scene, camera and switch changes of tests/walk_cases.py, and every read-back compared, bit for bit,
with what walk_cases.references computes without the product -- the oracle's frame, the host classifiers' counts, the host builds of the guide passes, the numpy
statement of the clear-distance tables.  What is held to them: the march / clear / see-through tile lists (renderer.cpp split_tiles), the costliest-first order
(tile_order), a grid's live cells, its clear-distance tables of both reaches, the majorant tables, the decoded float atlas, the path-seed table, the recorded
trace() calls (LaunchInputs::same_launch_as).  A field missing from one of their keys renders sky where there is smoke, or drops march steps that count.

Four modes, each one test over the whole list:
  all           after every step: frame and classes, features, expected0, expected1, both tables
  guides_first  the same, tables and guide passes first: a guide pass meets a new state before any colour launch has refreshed majorants, atlases or live cells
  one_each      at step k only read-back k mod 5: every cache sees several changes pile up before it is asked
  straddle      the steps that do not restart the frame: two trace() calls, the step, two more; the frame is the oracle's driven the same way and the frame of
                the same walk with coalesce_trace = 0

A mismatch is reported with the step, the mode and the read-back, and with what a FRESH renderer built directly in that state returns: fresh right = the walked
one is stale, fresh wrong too = a kernel or classifier bug.  The fresh renderer is a diagnostic, never the expectation.  tests/test_walk_host.py holds the list."""
import numpy as np
import pytest

import walk_cases as wc
from hk_common import bits

pytestmark = pytest.mark.gpu

WALK = wc.states()
GROUPS = ("frame", "features", "expected0", "expected1", "tables")          # what one_each cycles through; "frame" brings the classes


def _streams():
    import torch
    s = torch.cuda.Stream()
    return {"s1": s.cuda_stream, "_keep": s}


def _take(r, state, group):
    """{read-back: value} of one group, by the product calls of the issue's table"""
    if group == "frame":
        r.reset()
        r.render(wc.SPP)
        return {"frame": r.framebuffer(), "classes": (r.last_sky_tiles, r.last_see_through_tiles)}
    if group == "features":
        r.render_features(wc.FEATURE_SPP)
        return {"features": r.features()}
    if group in ("expected0", "expected1"):
        r.expected_field = int(group[-1])
        r.render_features_expected(wc.RAYS)
        return {group: r.features()}
    out = {}
    for field in (0, 1):
        r.expected_field = field
        out["table%d" % (field + 1)] = r.expected_clear_table()
    return out


def _agrees(k, got, want, state):
    if k == "classes":
        return tuple(got) == tuple(want)
    if k.startswith("table"):
        return got.shape == want.shape and np.array_equal(got, want)
    m = wc.mask(state)                                                    # outside the tile set a buffer keeps what earlier steps left there
    return got.shape == want.shape and np.array_equal(bits(got)[m], bits(want)[m])


def _describe(k, got, want, state):
    if k == "classes":
        return "(clear, see-through) = %s, reference %s" % (tuple(got), tuple(want))
    if k.startswith("table"):
        return "shape %s, reference %s, %d cells differ" % (got.shape, want.shape, int((got != want).sum()) if got.shape == want.shape else -1)
    if got.shape != want.shape:
        return "shape %s, reference %s" % (got.shape, want.shape)
    bad = (bits(got) != bits(want)).any(-1) & wc.mask(state)
    ys, xs = np.nonzero(bad)
    tiles = sorted(set(((ys // 16) * ((state["size"][0] + 15) // 16) + xs // 16).tolist()))
    return "%d pixels differ, in tiles %s" % (int(bad.sum()), tiles[:12])


def _check(problems, mode, step, r, state, group, streams):
    got = _take(r, state, group)
    want = wc.references(state)
    for k, v in got.items():
        if _agrees(k, v, want[k], state):
            continue
        fresh = wc.build_renderer(state, streams)
        fv = _take(fresh, state, group)[k]
        fresh.close()
        verdict = "a fresh renderer in this state agrees with the reference: the walked one is STALE" if _agrees(k, fv, want[k], state) else \
            "a fresh renderer in this state disagrees too (%s): WRONG, not stale" % _describe(k, fv, want[k], state)
        problems.append("mode %s, after step %d '%s', read-back %s: %s -- %s" % (mode, step, WALK[step][0] if step >= 0 else "the start", k, _describe(k, v, want[k], state), verdict))


def _tolerance_mode(problems, mode, step, r):
    """under fast_math = 1 only this: the frame is finite and nothing was split off; the check is at the step back"""
    r.reset()
    r.render(wc.SPP)
    if not np.isfinite(r.framebuffer()).all() or (r.last_sky_tiles, r.last_see_through_tiles) != (0, 0):
        problems.append("mode %s, after step %d '%s': the tolerance mode's frame is not finite, or tiles were split off" % (mode, step, WALK[step][0]))


def _walk(mode, groups_of):
    streams = _streams()
    r = wc.build_renderer(wc.START, streams)
    problems = []
    if mode != "one_each":                                                # the start state itself, in the mode's order
        for g in groups_of(0):
            _check(problems, mode, -1, r, wc.START, g, streams)
    for i, (name, change, targets, straddle, before, after) in enumerate(WALK):
        wc.apply_change(r, after, change, streams, before)
        if after["fast_math"]:
            _tolerance_mode(problems, mode, i, r)
            continue
        for g in groups_of(i):
            _check(problems, mode, i, r, after, g, streams)
    r.close()
    assert not problems, "%d mismatches; the first ones:\n%s" % (len(problems), "\n".join(problems[:8]))


def test_all():
    _walk("all", lambda i: ("frame", "features", "expected0", "expected1", "tables"))


def test_guides_first():
    _walk("guides_first", lambda i: ("tables", "expected1", "expected0", "features", "frame"))


def test_one_each():
    _walk("one_each", lambda i: (GROUPS[i % 5],))


def test_straddle():
    """steps that do not restart the frame (walk_cases straddle = True), on a split view: two recorded trace() calls, the step, two more.  The other steps are
    applied without a look, so the walk is the same walk."""
    streams = _streams()
    lazy, eager = wc.build_renderer(wc.START, streams), wc.build_renderer(wc.START, streams)
    eager.coalesce_trace = 0
    problems, n = [], 0
    for i, (name, change, targets, straddle, before, after) in enumerate(WALK):
        frames = []
        for r in (lazy, eager):
            if straddle:
                r.reset()
                r.trace()
                r.trace()
            wc.apply_change(r, after, change, streams, before)
            if straddle:
                r.trace()
                r.trace()
                r.synchronize()
                frames.append((r.framebuffer(), (r.last_sky_tiles, r.last_see_through_tiles), r.sample))
        if not straddle:
            continue
        n += 1
        want = wc.straddle_frame(before, after)
        for who, (fb, classes, sample) in zip(("coalesced", "one launch per call"), frames):
            if sample != 4:
                problems.append("mode straddle, step %d '%s', %s: the step restarted the frame (sample %d)" % (i, name, who, sample))
            if not _agrees("frame", fb, want, after):
                problems.append("mode straddle, step %d '%s', %s: %s against the oracle driven the same way" % (i, name, who, _describe("frame", fb, want, after)))
            if classes != wc.tile_classes(after):
                problems.append("mode straddle, step %d '%s', %s: (clear, see-through) = %s, reference %s" % (i, name, who, classes, wc.tile_classes(after)))
        if not _agrees("frame", frames[0][0], frames[1][0], after):
            problems.append("mode straddle, step %d '%s': coalesced != one launch per call, %s" % (i, name, _describe("frame", frames[0][0], frames[1][0], after)))
    lazy.close()
    eager.close()
    assert n >= 25
    assert not problems, "%d mismatches; the first ones:\n%s" % (len(problems), "\n".join(problems[:8]))
