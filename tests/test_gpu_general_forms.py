"""GPU: the GENERAL copy of the hot pair in every path-tracing kernel instance that ships, against the oracle.

Each kernel of variants 0, 1, 2 and 4 carries march + collide twice (vr_pathtrace.h, kCleanForms): the clean form, and one copy of the general form -- float inside
tests, a NaN guard on the density tap, a full division -- that runs in every scheduler iteration in which the wavefront holds a path on a segment begin_segment did
not mark clean (vr_trace.h seg_clean).  The clean lanes of such a wavefront go through it too, so it also holds the blocked-shadow shortcut, the 32-bit gather
offsets, the paired-atlas taps and the blocked majorant index.  A camera 36 000 volume widths away starts its segments at |ipos| > 2^20 voxels: not clean, while the
scatter and shadow segments that begin inside the volume are.  Every frame below is rendered from there by the instance named in ROWS -- each variant, with and
without a transfer function, both addressing forms where a variant has two, the instrumented (STATS) twins and the tolerance-mode builds -- and, the tolerance mode
apart, must be the oracle's bit for bit.  tests/test_host_kernel.py runs the same 14 configurations of the lane code, compiled for the host, on the CPU."""
import numpy as np
import pytest

from hk_common import bits as _bits
import scenes
from test_gpu_parity import FLAG_VARIANTS

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 56, 6      # ragged in both directions against the 16x16 tiles and the 8x8 work units
FAR = FLAG_VARIANTS["camera_very_far"][1]
CAMERA = ("cam_pos", "cam_dir", "cam_up", "cam_fov")

# row -> (config, transfer function on top, majorant_layout, expected kernel_variant, the wide_addressing values the variant has a build for)
ROWS = {
    "c2": ("c2", False, 0, 0, (0, 1)),
    "c3": ("c3", False, 0, 0, (0, 1)),                       # (the config brings its LUT)
    "c4": ("c4:64", False, 0, 1, (0, 1)),
    "c4_lut": ("c4:64", True, 0, 1, (0, 1)),
    "c5": ("c5:64", False, 0, 2, (0,)),
    "c5_lut": ("c5:64", True, 0, 2, (0,)),
    "c5_blocked": ("c5:64", False, 1, 4, (0,)),
    "c5_blocked_lut": ("c5:64", True, 1, 4, (0,)),
}
ROW_FORMS = [(row, wide) for row in ROWS for wide in ROWS[row][4]]
PLAIN_FORMS = [(row, wide) for row, wide in ROW_FORMS if not (ROWS[row][1] or row == "c3")]      # instances 0, 0w, 1, 1w, 2, 4 without a transfer function
_ids = lambda v: "%s-%s" % (v[0], "addresses64" if v[1] else "offsets32") if isinstance(v, tuple) else None
SCHED_DEFAULT = [64, 0, 56, 0, 60, 60, 64, 0]
_made = {}
_frames = {}


def _assert_same(got, want, what):
    nbad = int((_bits(got) != _bits(want)).any(-1).sum())
    assert nbad == 0, "%s: %d pixels differ from the oracle (relative L2 %.3e)" % (what, nbad, scenes.rel_l2(got[..., :3], want[..., :3]))


def _scene(row):
    """(HIP renderer, oracle renderer, the scene's own camera, bounces and albedo): built once per (config, transfer function); the rows that differ in the majorant layout share it"""
    config, lut = ROWS[row][:2]
    if (config, lut) not in _made:
        r, o = scenes.hip_scene(config, W, H), scenes.oracle_scene(config, W, H)
        if lut:
            r.load_transferfunc(scenes.LUT)
            o.load_transferfunc(scenes.LUT)
        own = {k: getattr(o, k) for k in CAMERA + ("bounces", "albedo")}      # (both renderers are configured alike)
        _made[(config, lut)] = (r, o, own)
    return _made[(config, lut)]


def _oracle_frame(row, camera, shadow_tail=False, seed=None):
    """The oracle's frame of the row's scene from the far camera or the scene's own; rendered once, shared by the instances and left unchanged"""
    config, lut = ROWS[row][:2]
    key = (config, lut, camera, shadow_tail, seed)
    if key not in _frames:
        _, o, own = _scene(row)
        keep = dict(bounces=o.bounces, albedo=o.albedo, seed=o.seed)
        for k in CAMERA:
            setattr(o, k, FAR.get(k, own[k]) if camera == "far" else own[k])
        if shadow_tail:
            o.bounces, o.albedo = 1000, (1.0, 1.0, 1.0)
        if seed is not None:
            o.seed = seed
        o.reset()
        fb = o.render(SPP).copy()
        if camera == "far":
            # (a) on the oracle's side the camera stands beyond 2^20 voxels in index space: its segments are not clean
            ipos = np.array(o.params().vol_density_inv_transform, np.float32).reshape(4, 4).T @ np.array([*o.cam_pos, 1.0], np.float32)
            far_enough = bool(np.abs(ipos[:3]).max() > 2.0 ** 20)
        else:
            far_enough = False
        for k, v in keep.items():
            setattr(o, k, v)
        fb.setflags(write=False)
        _frames[key] = (fb, far_enough)
    return _frames[key]


def _select(row, wide, camera="far", shadow_tail=False):
    """The row's HIP renderer with the instance selected and the camera placed; (c): the intended instance serves the next launch"""
    _, _, layout, variant, _ = ROWS[row]
    r, _, own = _scene(row)
    r.majorant_layout = layout
    r.wide_addressing = wide
    r.fast_math = 0
    r.set_sched(SCHED_DEFAULT)
    for k in CAMERA:
        setattr(r, k, FAR.get(k, own[k]) if camera == "far" else own[k])
    r.bounces = 1000 if shadow_tail else own["bounces"]
    r.albedo = (1.0, 1.0, 1.0) if shadow_tail else own["albedo"]
    assert r.kernel_variant == variant, (row, r.kernel_variant)
    assert r.kernel_wide == (1 if (wide or variant >= 2) else 0)          # small tables: the switch decides; variants 2 and 4 always form 64-bit addresses
    assert r.kernel_variant_reason == 0
    return r


def _render(r):
    r.reset()
    r.render(SPP)
    return r.framebuffer().copy()


@pytest.mark.parametrize("form", ROW_FORMS, ids=_ids)
def test_general_copy_matches_oracle_and_the_clean_copies_take_over_again(form):
    row, wide = form
    want, far_enough = _oracle_frame(row, "far")
    assert far_enough                                                      # (a)
    assert want[..., 3].max() == 1.0 and want[..., 3].mean() > 0.01        # (b) the segments do march: the volume is hit
    r = _select(row, wide)                                                 # (c)
    _assert_same(_render(r), want, "%s, wide_addressing %d, far camera" % form)      # (d)
    # back to the scene's own camera on the same renderer: every segment is clean again, the wavefronts return to the clean copies
    near, _ = _oracle_frame(row, "own")
    assert near[..., 3].max() == 1.0
    r = _select(row, wide, camera="own")
    _assert_same(_render(r), near, "%s, wide_addressing %d, the scene's own camera afterwards" % form)


@pytest.mark.parametrize("form", [(row, wide) for row in ("c2", "c4") for wide in (0, 1)], ids=_ids)
def test_shadow_shortcut_in_the_general_copy(form):
    """1000 bounces at albedo 1: most shadow rays end blocked, where collide_finish takes its shortcut -- here in the general copy, which the clean shadow lanes of a
    wavefront go through while another of its lanes is on a camera segment from far away."""
    row, wide = form
    want, far_enough = _oracle_frame(row, "far", shadow_tail=True)
    assert far_enough
    assert want[..., 3].max() == 1.0 and want[..., 3].mean() > 0.01
    r = _select(row, wide, shadow_tail=True)
    _assert_same(_render(r), want, "%s, wide_addressing %d, 1000 bounces at albedo 1" % form)


@pytest.mark.parametrize("form", ROW_FORMS, ids=_ids)
def test_instrumented_twins_run_the_same_general_copy(form):
    """The STATS build of every instance, selected as test_gpu_parity.py::test_instrumented_and_tolerance_kernels_are_consistent selects it: the plain kernel's
    far-camera frame, bit for bit."""
    row, wide = form
    r = _select(row, wide)
    plain = _render(r)
    assert plain[..., 3].max() == 1.0
    r.sched_stats(True)
    try:
        got = _render(r)
    finally:
        st = r.sched_stats(False, read=True)
    assert st["waves"] > 0
    assert np.array_equal(_bits(got), _bits(plain)), "instrumented kernel, %s, wide_addressing %d" % form


@pytest.mark.parametrize("form", PLAIN_FORMS, ids=_ids)
def test_tolerance_mode_general_copy(form):
    """fast_math = 1 from the far camera: every value finite, one frame whatever the scheduler does, and no further from the oracle's frame than a second oracle
    frame of the scene at the same spp with another seed is -- the Monte-Carlo noise of the reference, computed here."""
    row, wide = form
    want, far_enough = _oracle_frame(row, "far")
    other, _ = _oracle_frame(row, "far", seed=20261)
    assert far_enough and want[..., 3].max() == 1.0
    noise = scenes.rel_l2(other[..., :3], want[..., :3])
    assert noise > 0
    r = _select(row, wide)
    try:
        r.fast_math = 1
        fast = _render(r)
        assert np.isfinite(fast).all()
        for thr in ([64, 0, 56, 32, 60, 60, 64, 0], [8, 0, 8, 40, 8, 8, 8, 0], [1, 66, 1, 1, 1, 1, 1, 0]):
            r.set_sched(thr)
            assert np.array_equal(_bits(_render(r)), _bits(fast)), ("tolerance-mode kernel, scheduler", form, thr)
        err = scenes.rel_l2(fast[..., :3], want[..., :3])
        print("tolerance mode %s wide %d: relative L2 to the oracle %.4e, between two oracle seeds %.4e" % (row, wide, err, noise))
        assert err <= noise, (form, err, noise)
    finally:
        r.fast_math = 0
        r.set_sched(SCHED_DEFAULT)
