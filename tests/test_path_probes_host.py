"""CPU: the per-path layer of the device code (volren_amd/csrc/vr_path_probe.h: the inline functions of vr_trace.h that turn a pixel into a ray, a ray into a
segment and a segment into a collision, in the compile-time forms the kernels instantiate), compiled for the host by tests/hostkernel/path_probe_host.cpp,
against the oracle's batch forms (orc_batch_rng ... orc_batch_segment) -- word for word, on the catalogue of tests/path_cases.py: not only along the rays a
frame casts.  The host build's trace sink checks every majorant and tap access against the extent of its table.  tests/test_gpu_path_probes.py runs the same
items on the device."""
import os
import re

import numpy as np
import pytest

import hk_path as hp
import path_cases as pc
import scenes
from oracle import binding as ob


def _check(s, o, kind, form, items):
    got, want = s.path_probe(kind, form, items), o.path_probe(kind, items)
    assert pc.same(kind, got, want), "form %d: %s" % (form, pc.first_difference(kind, items, got, want))
    assert hp.violations() == 0
    return got


@pytest.fixture(scope="module")
def c2():
    o = scenes.oracle_scene("c2", 16, 16)
    s = hp.Scene(o)
    yield o, s
    s.close()


def test_budget_is_stated_once_per_side():
    """ORC_SEGMENT_BUDGET (oracle/volren_oracle.h) = the binding's figure = vr_path_probe.h's kPathSegmentBudget, and the device runs twice as many passes"""
    text = open(os.path.join(scenes.ROOT, "oracle", "volren_oracle.h")).read()
    stated = re.findall(r"#define\s+ORC_SEGMENT_BUDGET\s+(\d+)", text)
    assert len(stated) == 1 and int(stated[0]) == ob.OracleRenderer.segment_budget() == 4096
    assert hp.constants() == (int(stated[0]), 2 * int(stated[0]))


def test_rng(c2):
    """tea32, path_seed, rng, rng_skip9 against the oracle and against NumPy integer arithmetic; the solved states draw exactly 0 and 1 - 2^-24"""
    o, s = c2
    items = pc.rng_items()
    assert (1 << 20) + 4 <= len(items) <= (1 << 20) + 1024
    got = _check(s, o, pc.RNG, 0, items)
    ref = pc.np_rng_reference(items)
    assert pc.same(pc.RNG, got, ref), pc.first_difference(pc.RNG, items, got, ref)
    for low, value in ((0, 0.0), (0xFFFFFF, float(pc.ONE_M))):
        st = np.zeros((256, 8), np.uint32)
        st[:, 0] = pc.states_with_first_draw(low)
        assert len(set(st[:, 0].tolist())) == 256
        assert (o.path_probe(pc.RNG, st)[:, 0].view(np.float32) == np.float32(value)).all()


@pytest.mark.parametrize("frame", pc.CAMERA_FRAMES, ids=["%dx%d" % f for f in pc.CAMERA_FRAMES])
@pytest.mark.parametrize("camera", sorted(pc.CAMERAS))
def test_camera(camera, frame):
    """do_new's ray against pixel_sample's, and the RNG state after the two jitter draws"""
    o = pc.camera_scene(True, camera, *frame, seed=-7 if camera == "top_down" else 42)
    s = hp.Scene(o)
    items = pc.camera_items(*frame)
    assert len(items) == 3 * (frame[0] * frame[1] if frame[0] * frame[1] < 4096 else 4)
    got = _check(s, o, pc.CAMERA, 0, items)
    if camera not in ("fov0",):
        assert np.isfinite(got[:, :3].view(np.float32)).all()
    with pytest.raises(hp.Refused):
        s.path_probe(pc.CAMERA, 0, np.array([[frame[0], 0, 1, 0]], np.uint32))      # a pixel outside the frame is refused: do_new would skip it
    s.close()


@pytest.mark.parametrize("crop", [False, True])
def test_box(crop):
    o = scenes.oracle_scene("c2", 16, 16)
    if crop:
        for k, v in pc.CROP.items():
            setattr(o, k, v)
    p = o.params()
    s = hp.Scene(o)
    items = pc.box_items(p.vol_bb_min[:], p.vol_bb_max[:])
    assert 1 << 16 < len(items) <= 1 << 17
    got = _check(s, o, pc.BOX, 0, items)
    assert 0.2 < got[:, 0].mean() < 0.8                                             # hits and misses both
    s.close()


def test_phase(c2):
    o, s = c2
    _check(s, o, pc.PHASE, 0, pc.phase_items())


def test_dda_step(c2):
    o, s = c2
    general, clean = pc.dda_items(), pc.dda_items(clean=True)
    _check(s, o, pc.DDA, 0, general)
    _check(s, o, pc.DDA, 0, clean)
    _check(s, o, pc.DDA, 1, clean)
    ri = clean[:, 3:6].view(np.float32)
    assert np.isinf(ri).any() and not np.isnan(ri).any() and np.isnan(general[:, :6].view(np.float32)).any()
    with pytest.raises(hp.Refused):
        s.path_probe(pc.DDA, 1, general)                                            # NaN is outside the CLEAN form's contract


def _f(words):
    return np.ascontiguousarray(words).view(np.float32)


@pytest.mark.parametrize("name", sorted(pc.SEGMENT_SCENES))
def test_segments(name):
    """One whole segment of the hot pair -- hot_init, begin_segment, march and collide passes in the form the item's seg_clean picks -- per compiled instance the
    scene serves, against the oracle's bounded trackers.  First, from the oracle's outputs alone, the conditions that make the sets worth running."""
    cfg = pc.SEGMENT_SCENES[name]
    o, compared, bounded = pc.segment_case(name)
    glob, thin = o.integrator != 0, cfg.get("thin_medium", False)
    # ---- budget: at most 1 % of any compared set unfinished ----
    for sn, (items, want) in compared.items():
        share = float((want[:, 0] == 3).mean())
        assert share <= pc.BUDGET_CAP, "scene %s set %s: %.2f %% of the items exhaust the oracle's budget" % (name, sn, 100 * share)
    assert set(compared) | set(bounded) == set(pc.ALL_SETS) | {"stall"} and len(bounded["stall"][0]) == 64 * 4
    # ---- coverage: the sets 1. - 8. (not the stall set), over what the oracle finishes ----
    sets = [v for g in (compared, bounded) for sn, v in g.items() if sn != "stall"]
    items, want = np.concatenate([v[0] for v in sets]), np.concatenate([v[1] for v in sets])
    done = want[:, 0] != 3
    items, want = items[done], want[done]
    for kind in (0, 1):
        counts = np.bincount(want[items[:, 7] == kind, 0], minlength=3)
        assert all(c >= 200 for c in counts[:3]), "scene %s kind %d: statuses %s" % (name, kind, counts.tolist())
    # null collisions, on the camera / scatter segments: there every tentative collision but the real one that ends the segment is null (a shadow segment's real
    # collisions that survive the roulette are not told apart from null ones in the oracle's count)
    cam = items[:, 7] == 0
    nulls = want[cam, 5].astype(np.int64) - (want[cam, 0] == 2)
    assert int((nulls >= 1).sum()) >= 100
    if not glob:
        assert int(((want[:, 3] == 12) & (want[:, 5] > 0)).sum()) >= 100              # back on DDA level 3 after a collision took it down
        low = int(((want[:, 3] < 4) & (want[:, 0] != 0)).sum())
        if thin:
            # the scene has no such segment: at scales 2^-16 and 2^-17 a segment collides on a first free flight of a few 2^-24 only (the *_first_draw and
            # *_small_draw sets), the draw after a null collision is an ordinary one, and no segment of the sets collides twice -- one collision leaves level 1
            assert low == 0 and int(want[:, 5].max()) == 1
        else:
            assert low >= 100
    one = np.float32(1.0).view(np.uint32)
    if o.lut is not None:
        assert int(((want[:, 0] == 2) & cam & (want[:, 7:10] != one).any(1)).sum()) >= 100
    else:
        assert not want[:, 7:10].any()
    if o.emission is not None:
        assert int((_f(want[:, 10:13]) != 0).any(1).sum()) >= 100
    else:
        assert not want[:, 10:13].any()
    # ---- the product's code, every instance the scene serves ----
    s = hp.Scene(o, pc.host_flags(name))
    before = hp.accesses()
    for form in cfg["forms"]:
        res = pc.check_segments(name, s.path_probe, form)
        clean = np.concatenate([res[sn][:, 13] for sn in res])
        hit = np.concatenate([res[sn][:, 0] for sn in res]) != 0
        assert int(((clean == 0) & hit).sum()) >= 100, "scene %s: %d segments that are not clean" % (name, int(((clean == 0) & hit).sum()))
        if not glob:
            assert int(clean.sum()) >= 10000
    # (the global-majorant pair under a LUT reads no majorant table and its trilinear corners from the decoded float atlas, which the sink does not see)
    assert (hp.accesses() > before or (glob and o.lut is not None)) and hp.violations() == 0
    # ---- refusals: every other instance, with the reason ----
    assert s.instance in cfg["forms"] and 6 in cfg["forms"]
    probe = next(iter(compared.values()))[0][:4] if compared else bounded["stall"][0][:4]
    for form in range(7):
        if form in cfg["forms"]:
            continue
        with pytest.raises(hp.Refused) as e:
            s.path_probe(pc.SEGMENT, form, probe)
        assert "instance" in str(e.value), (form, str(e.value))
    with pytest.raises(hp.Refused):
        s.path_probe(pc.SEGMENT, 7, probe)
    s.close()


def test_reasons_of_the_refusals():
    """what a refusal says: the density scale, the integrator, the grids"""
    for name, word in (("c2-scale-2^-17", "density scale"), ("c2-global", "integrator"), ("emission-other-layout-linear", "paired atlas"), ("c4:64", "another kind")):
        o = pc.segment_case(name)[0]
        s = hp.Scene(o, pc.host_flags(name))
        with pytest.raises(hp.Refused) as e:
            s.path_probe(pc.SEGMENT, 4, pc.segment_case(name)[2]["stall"][0][:1])
        assert word in str(e.value), (name, str(e.value))
        s.close()
