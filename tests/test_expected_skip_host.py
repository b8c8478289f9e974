"""CPU: empty-space skipping in the expected-value feature pass.  The clear-distance table (volren_amd/csrc/vr_clear.h), host-compiled
(tests/hostkernel/expected_skip_host.cpp), against a numpy statement of its definition (tests/hk_expected_skip.py spec_table); the march that skips
by it (vr_expected.h) against the march that runs every step, bit for bit, with every dropped step audited; and the work it has left."""
import numpy as np
import pytest

import encoder_ref
import hk_expected as he
import hk_expected_skip as hs
import scenes
from hk_common import same as _same

W, H = 64, 48
SCENES = ("c1", "c3", "c4_64", "c5_64")


# ---- 1: the table ------------------------------------------------------------------------------------------------------------------------------------
def _scene_of(grid, w=16, h=12):
    from oracle import binding as ob
    o = ob.OracleRenderer(w, h)
    o.set_volume(grid)
    return o


def _blobs_60x44x52():
    """a dense fp16 grid of 60 x 44 x 52 voxels (x, y, z): partial cells at the upper edge of every axis, three blobs, most of it empty"""
    z, y, x = np.meshgrid(np.arange(52), np.arange(44), np.arange(60), indexing="ij")
    v = np.zeros((52, 44, 60), np.float32)
    for cx, cy, cz, r in ((14.0, 12.0, 30.0, 6.0), (57.0, 41.0, 49.0, 4.0), (30.0, 22.0, 3.0, 2.5)):
        v += np.maximum(0.0, 1.0 - ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (r * r)).astype(np.float32)
    return v.astype(np.float16)


def _marked_40():
    """40^3 dense fp16 voxels, all +0 but four: a non-zero voxel on a cell face (the first of cell 1 along x: it lies in the grown box of cell 0 too), one in
    the last corner voxel of the grid, a -0 and a NaN"""
    v = np.zeros((40, 40, 40), np.float16)
    v[20, 20, 8] = 1.0
    v[39, 39, 39] = 0.5
    v[36, 4, 20] = -0.0
    v[4, 36, 4] = np.nan
    return v


def _line_of_300_bricks():
    """300 x 1 x 1 bricks, one non-zero voxel in the first: the byte of brick i is min(255, i)"""
    from oracle import binding as ob
    n = 300
    rng = np.zeros(n, np.uint32)
    rng[0] = 0x3C00 << 16                                  # range (0, 1) in fp16
    atlas = np.zeros((8, 8, 8), np.uint8)
    atlas[3, 3, 0] = 255
    g = ob.Grid()
    g.set(np.eye(4, dtype=np.float32).reshape(16), (n, 1, 1), (0.0, 1.0), 1, np.zeros(n, np.uint32), rng, (8, 8, 8), atlas.reshape(-1), [])
    return g


TABLE_CASES = {
    "c1": lambda: scenes.oracle_scene("c1", 16, 12),
    "c3": lambda: scenes.oracle_scene("c3", 16, 12),           # under a LUT the host scene decodes the atlas to floats: the table reads those
    "c4_64": lambda: scenes.oracle_scene("c4_64", 16, 12),
    "c5_64": lambda: scenes.oracle_scene("c5_64", 16, 12),
    "dense_60x44x52": lambda: _scene_of(encoder_ref.encode_dense_fp16(_blobs_60x44x52())),
    "marked_40": lambda: _scene_of(encoder_ref.encode_dense_fp16(_marked_40())),
    "zeros_24": lambda: _scene_of(encoder_ref.encode_dense_fp16(np.zeros((24, 24, 24), np.float16))),
    "bricks_300x1x1": lambda: _scene_of(_line_of_300_bricks()),
}


@pytest.mark.parametrize("case", sorted(TABLE_CASES))
def test_the_host_table_is_the_numpy_statement_byte_for_byte(case):
    o = TABLE_CASES[case]()
    got, want = hs.table(o), hs.spec_table(o.density)
    assert got.shape == want.shape and np.array_equal(got, want), (case, int((got != want).sum()))
    print("%s: %s cells, %d not clear, largest byte %d" % (case, "x".join(str(v) for v in got.shape[::-1]), int((got == 0).sum()), int(got.max())))
    if case == "zeros_24":
        assert got.shape == (3, 3, 3) and (got == 255).all()
    elif case == "bricks_300x1x1":
        assert got.shape == (1, 1, 300) and np.array_equal(got.reshape(-1), np.minimum(255, np.arange(300)))
    elif case == "dense_60x44x52":
        assert got.shape == (7, 6, 8) and (got == 0).any() and (got >= 2).any()
    elif case == "marked_40":
        assert got.shape == (5, 5, 5)
        assert got[2, 2, 0] == 0 and got[2, 2, 1] == 0 and got[2, 2, 2] == 1             # the face voxel marks both cells it touches
        assert got[4, 4, 4] == 0 and got[4, 0, 2] == 0 and got[0, 4, 0] == 0             # the corner voxel, the -0, the NaN
        assert (got == 0).sum() == 5 and got.max() >= 2
    else:
        assert (got == 0).any() and (got > 0).any()


# ---- 2: the same bits, and nothing dropped that counts ------------------------------------------------------------------------------------------------
def _check(o, rays, what, expect_no_skip=False):
    """skip off, on and audited give the same frame and the same sub-ray records; the audit finds no dropped step with sigma > 0; off fetches every step"""
    off = hs.expected_pass(o, rays, 0)
    on = hs.expected_pass(o, rays, 1)
    audit = hs.expected_pass(o, rays, 2)
    assert _same(off[0], he.expected_pass(o, rays)), what                               # the harness's own entry point, which knows no table
    for got in (on, audit):
        assert _same(got[0], off[0]), (what, "frame")
        assert np.array_equal(got[1], off[1]) and np.array_equal(got[2], off[2]) and _same(got[3], off[3]), (what, "sub-ray records")
    w0, w1, w2 = off[4], on[4], audit[4]
    assert w2["audit"] == 0, (what, w2)
    assert w0["fetched"] == w0["steps"] == int(off[2].sum()) and w0["reads"] == 0 and w0["rays"] == int((off[1] > 0).sum()), (what, w0)
    assert w1["steps"] == w0["steps"] and w1["rays"] == w0["rays"] and {k: w2[k] for k in ("rays", "steps", "fetched", "reads")} == {k: w1[k] for k in ("rays", "steps", "fetched", "reads")}
    if expect_no_skip:
        assert w1["fetched"] == w1["steps"] and w1["reads"] == 0, (what, w1)
    else:
        assert w1["fetched"] <= w1["steps"], (what, w1)
    return off, w1


@pytest.mark.parametrize("rays", (1, 2))
@pytest.mark.parametrize("name", SCENES)
def test_skipping_changes_no_bit(name, rays):
    off, w = _check(scenes.oracle_scene(name, W, H), rays, (name, rays))
    assert (off[0][..., 3] > 0).sum() > 500 and w["fetched"] < w["steps"]


def _inside(o):
    o.cam_pos, o.cam_dir, o.cam_fov = (0.05, 0.0, -0.1), (0.4, 0.2, 1.0), 80.0


def _far(o):
    o.cam_pos, o.cam_fov = tuple(36000.0 * x for x in o.cam_pos), 40.0 / 36000.0


def _clip(o):
    o.vol_clip_min, o.vol_clip_max = (0.0, 0.0, 0.0), (1.0, 0.45, 1.0)


def _scale_zero(o):
    o.density_scale = 0.0


def _scale_negative(o):
    o.density_scale = -3.0


def _window_left_zero(o):
    o.tf_window_left = 0.0


def _window_left_below_zero(o):
    o.tf_window_left = -0.25


EDGE = (("c1", _inside), ("c1", _far), ("c1", _clip), ("c1", _scale_zero), ("c4_64", _scale_zero), ("c1", _scale_negative), ("c3", _scale_negative),
        ("c3", _window_left_zero), ("c3", _window_left_below_zero))


@pytest.mark.parametrize("name,case", EDGE, ids=["%s%s" % (n, f.__name__) for n, f in EDGE])
def test_skipping_changes_no_bit_at_the_edges(name, case):
    """the camera inside the volume; 36 000 widths away (where the coordinates are too coarse to leap: one step at a time); test_expected_host's clip box;
    a density scale of 0 and a negative one; a LUT window that starts at 0 and one that starts below it"""
    o = scenes.oracle_scene(name, 32, 24)
    case(o)
    _, w = _check(o, 2, (name, case.__name__))
    print("%s %s: %s" % (name, case.__name__, w))


def test_a_lut_with_alpha_at_density_zero_skips_nothing():
    """empty space is not empty when the LUT's first entry has alpha > 0: the launch marches every step and reads no table"""
    o = scenes.oracle_scene("c3", 32, 24)
    lut = o.lut.copy()
    lut[0, 3] = 0.25
    o.lut = lut
    off, w = _check(o, 2, "alpha(0) > 0", expect_no_skip=True)
    through = (off[1] > 0).any(axis=2)
    assert through.sum() > 100 and (off[0][..., 3] > 0)[through].all()                # every ray through the box collides with the haze


# ---- 3: the work that is left -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_the_steps_that_still_fetch(name):
    """64x48, 1 ray.  The steps that fetch their corners are within 1 % of the float64 count of "the midpoint's cell is not clear, or outside the table" over
    the steps each sub-ray reached (float32 against float64 at cell borders), and at most half of the steps reached.  Measured:
                 steps reached   fetched   share    float64 count   table reads
      c1               135 667    49 253   0.363           49 253        78 612
      c3               137 770    50 420   0.366           50 420        80 271
      c4_64            101 022    46 005   0.455           46 005        97 776
      c5_64            132 407    26 512   0.200           26 512       102 582
    (The reads stay close to the steps on the two 64^3 grids: their clear cells are one or two cells deep, so a leap is rarely longer than the step itself.)"""
    o = scenes.oracle_scene(name, W, H)
    out, m, steps, T, w = hs.expected_pass(o, 1, 1)
    want = hs.spec_fetched(o, hs.spec_table(o.density), steps, 1)
    print("%s: steps reached %d, fetched %d (%.3f), float64 count %d, table reads %d" % (name, w["steps"], w["fetched"], w["fetched"] / w["steps"], want, w["reads"]))
    assert abs(w["fetched"] - want) <= 0.01 * want, (w, want)
    assert w["fetched"] <= 0.5 * w["steps"], w
    assert 0 < w["reads"] <= w["steps"]
