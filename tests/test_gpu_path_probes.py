"""GPU: the per-path layer on the device against the oracle, word for word -- Renderer.path_probe (include/volren_amd.h vr_path_probe) runs the inline functions of
vr_trace.h that turn a pixel into a ray, a ray into a segment and a segment into a collision, in the compile-time forms the kernels instantiate: the rcp_newton
branch of rcp3_exact under intersect_box, the unrolled tea32, v_cvt_flr / v_min3 of the CLEAN forms, div_core in march_finish, the fast tricubic tap.  The items
are the catalogue of tests/path_cases.py and nothing else; tests/test_path_probes_host.py runs the same items through the host build of the same header and
holds the sets to their budget and coverage conditions."""
import numpy as np
import pytest

import path_cases as pc
import scenes

pytestmark = pytest.mark.gpu


def _check(r, o, kind, form, items):
    got, want = r.path_probe(kind, form, items), o.path_probe(kind, items)
    assert pc.same(kind, got, want), "form %d: %s" % (form, pc.first_difference(kind, items, got, want))
    return got


def _refused(r, kind, form, items):
    import volren_amd
    with pytest.raises(volren_amd.VolrenError) as e:
        r.path_probe(kind, form, items)
    return str(e.value)


def test_rng():
    o, r = scenes.oracle_scene("c2", 16, 16), scenes.hip_scene("c2", 16, 16)
    items = pc.rng_items()
    got = _check(r, o, pc.RNG, 0, items)
    ref = pc.np_rng_reference(items)
    assert pc.same(pc.RNG, got, ref), pc.first_difference(pc.RNG, items, got, ref)


@pytest.mark.parametrize("camera", sorted(pc.CAMERAS))
def test_camera(camera):
    for frame in pc.CAMERA_FRAMES:
        seed = -7 if camera == "top_down" else 42
        o, r = pc.camera_scene(True, camera, *frame, seed=seed), pc.camera_scene(False, camera, *frame, seed=seed)
        _check(r, o, pc.CAMERA, 0, pc.camera_items(*frame))
        assert "outside the frame" in _refused(r, pc.CAMERA, 0, np.array([[frame[0], 0, 1, 0]], np.uint32))
        r.close()


@pytest.mark.parametrize("crop", [False, True])
def test_box(crop):
    o, r = scenes.oracle_scene("c2", 16, 16), scenes.hip_scene("c2", 16, 16)
    if crop:
        for k, v in pc.CROP.items():
            setattr(o, k, v)
            setattr(r, k, v)
    p = o.params()
    _check(r, o, pc.BOX, 0, pc.box_items(p.vol_bb_min[:], p.vol_bb_max[:]))


def test_phase():
    o, r = scenes.oracle_scene("c2", 16, 16), scenes.hip_scene("c2", 16, 16)
    _check(r, o, pc.PHASE, 0, pc.phase_items())


def test_dda_step():
    o, r = scenes.oracle_scene("c2", 16, 16), scenes.hip_scene("c2", 16, 16)
    general, clean = pc.dda_items(), pc.dda_items(clean=True)
    _check(r, o, pc.DDA, 0, general)
    _check(r, o, pc.DDA, 0, clean)
    _check(r, o, pc.DDA, 1, clean)
    assert "CLEAN" in _refused(r, pc.DDA, 1, general)


@pytest.mark.parametrize("name", sorted(pc.SEGMENT_SCENES))
def test_segments(name):
    """every instance the scene serves on the scene's sets: the compared ones in full, the bounded ones (stall set, over-budget classes) where the oracle finished;
    every other instance is refused with the reason"""
    cfg = pc.SEGMENT_SCENES[name]
    r = pc.segment_scene(name, False)
    for form in cfg["forms"]:
        pc.check_segments(name, r.path_probe, form)
    probe = pc.segment_case(name)[2]["stall"][0][:4]
    for form in range(7):
        if form not in cfg["forms"]:
            why = _refused(r, pc.SEGMENT, form, probe)
            assert "cannot serve" in why and "instance" in why, (form, why)
    assert "out of range" in _refused(r, pc.SEGMENT, 7, probe)
    r.close()
