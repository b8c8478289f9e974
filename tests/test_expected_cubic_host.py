"""CPU: the expected-value feature pass on the tracker's field (vr_set_int "expected_field" 1: volren_amd/csrc/vr_cubic.h and vr_expected.h CUBIC),
host-compiled (tests/hostkernel/expected_cubic_host.cpp).  The cubic B-spline lookup against known answers and a float64 statement; the whole pass
against a float64 statement; the coverage against the path tracer's own, which is what the feature is for; empty-space skipping with the table of
reach 2; and the LUT case, where the setting changes nothing."""
import numpy as np
import pytest

import encoder_ref
import hk_expected as he
import hk_expected_cubic as hc
import hk_features
import scenes
from hk_common import same as _same

W, H = 64, 48
CH = ("albedo.r", "albedo.g", "albedo.b", "coverage", "normal.x", "normal.y", "normal.z", "depth")


def _scene_of(grid, w=8, h=8):
    from oracle import binding as ob
    o = ob.OracleRenderer(w, h)
    o.set_volume(grid)
    return o


def _brick_grid(vox):
    """hk_expected_cubic.brick_arrays as an oracle grid: integer voxel values 0..255 [z][y][x] that decode to themselves"""
    return hc.oracle_brick_grid(hc.brick_arrays(vox))


def _index(shape):
    return np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")      # z, y, x


# the tiny grids: a dense fp16 grid of 6 x 5 x 4 voxels and a brick grid of 2 x 1 x 1 bricks (x, y, z); `ramp`: (base, slope x, y, z) in voxel-index terms
GRIDS = {
    "dense_6x5x4": dict(shape=(4, 5, 6), const=0.75, ramp=(1.0, 0.5, 0.25, 2.0), make=lambda v: encoder_ref.encode_dense_fp16(v.astype(np.float16))),
    "bricks_2x1x1": dict(shape=(8, 8, 16), const=37.0, ramp=(3.0, 2.0, 5.0, 11.0), make=lambda v: _brick_grid(v)),
}
# largest |host build - float64 statement| over the points compared, measured with these tests (they print it): value, then the gradient's components
MEASURED_KNOWN = {("dense_6x5x4", "const"): (2.38e-07, 5.21e-08), ("dense_6x5x4", "ramp"): (1.73e-06, 9.54e-07),
                  ("bricks_2x1x1", "const"): (1.14e-05, 3.08e-06), ("bricks_2x1x1", "ramp"): (2.72e-05, 1.34e-05)}
MEASURED_CATALOGUE = {"dense_6x5x4": (1.80e-06, 1.04e-06), "bricks_2x1x1": (2.71e-05, 1.70e-05)}


def _tiny(name, kind):
    G = GRIDS[name]
    z, y, x = _index(G["shape"])
    b, sx, sy, sz = G["ramp"]
    vox = np.full(G["shape"], G["const"]) if kind == "const" else b + sx * x + sy * y + sz * z
    o = _scene_of(G["make"](vox))
    grid = hk_features.decoded_grid(o.density)
    assert np.array_equal(grid, vox.astype(np.float64))                     # the voxels decode to the numbers meant, exactly
    return o, grid


@pytest.mark.parametrize("kind", ("const", "ramp"))
@pytest.mark.parametrize("name", sorted(GRIDS))
def test_the_filter_returns_a_constant_and_a_ramp(name, kind):
    """At points two or more voxels inside, where all 64 taps lie in the grid: a constant field comes back with gradient 0, a linear ramp with its slope --
    the cubic B-spline reproduces linear functions.  The float64 statement to 1e-12 (relative to the field's largest value); the host build to four times its
    measured largest difference from the float64 statement (MEASURED_KNOWN)."""
    o, grid = _tiny(name, kind)
    nz, ny, nx = grid.shape
    rng = np.random.default_rng(11)
    p = np.concatenate([rng.uniform(2.0, np.array([nx, ny, nz]) - 2.0, (4000, 3)), np.array([[2.0, 2.0, 2.0], [nx - 2.0, ny - 2.0, nz - 2.0], [2.5, 2.5, 2.5]])]).astype(np.float32)
    p64 = p.astype(np.float64)
    val, g = hc.cubic(grid, p64)
    b, sx, sy, sz = GRIDS[name]["ramp"]
    if kind == "const":
        want, slope = np.full(len(p), GRIDS[name]["const"]), np.zeros(3)
    else:
        want, slope = b + sx * (p64[:, 0] - 0.5) + sy * (p64[:, 1] - 0.5) + sz * (p64[:, 2] - 0.5), np.array([sx, sy, sz])
    top = float(np.abs(grid).max())
    assert np.abs(val - want).max() <= 1e-12 * top and np.abs(g - slope[None, :]).max() <= 1e-12 * top
    hc.reset()
    got = hc.probe(o, p)
    assert hc.violations() == (0, 64 * len(p))                              # every tap inside its table
    dv, dg = float(np.abs(got[:, 0] - val).max()), float(np.abs(got[:, 1:] - g).max())
    print("%s %s: host - float64: value %.2e gradient %.2e" % (name, kind, dv, dg))
    m = MEASURED_KNOWN[(name, kind)]
    assert dv <= 4.0 * m[0] and dg <= 4.0 * m[1], (dv, dg)


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_the_lookup_over_the_point_catalogue(name):
    """hk_expected_cubic.catalogue on the ramp grids: t = 0 and the float below 1, brick faces from both sides, the borders from both sides, negative
    coordinates, -0, a denormal: the host build within four times its measured largest difference from the float64 statement (MEASURED_CATALOGUE).  A NaN or
    infinite coordinate gives NaN, +-2^30 gives +0 with gradient 0, and no tap of the whole catalogue leaves its table."""
    o, grid = _tiny(name, "ramp")
    nz, ny, nx = grid.shape
    pts = hc.catalogue((nx, ny, nz))
    hc.reset()
    got = hc.probe(o, pts)
    bad, taps = hc.violations()
    assert bad == 0 and taps == 64 * len(pts), (bad, taps)
    finite = np.isfinite(pts).all(axis=1)
    assert (~finite).sum() == 18 and np.isnan(got[~finite]).all()
    huge = finite & (np.abs(pts) >= 2.0 ** 30).any(axis=1)
    assert huge.sum() == 12 and not got[huge].any() and not np.signbit(got[huge]).any()
    val, g = hc.cubic(grid, pts[finite].astype(np.float64))
    dv, dg = float(np.abs(got[finite][:, 0] - val).max()), float(np.abs(got[finite][:, 1:] - g).max())
    print("%s: %d points, host - float64: value %.2e gradient %.2e" % (name, len(pts), dv, dg))
    m = MEASURED_CATALOGUE[name]
    assert dv <= 4.0 * m[0] and dg <= 4.0 * m[1], (dv, dg)
    # floor, not truncation: at x = -0.3 the lookup still reaches voxel 0 (fl = -1: taps -2 .. 1), and it is the float64 statement's value, not 0
    p = np.array([[-0.3, 2.5, 2.5]], np.float32)
    assert hc.probe(o, p)[0, 0] > 0 and abs(hc.probe(o, p)[0, 0] - hc.cubic(grid, p.astype(np.float64))[0][0]) <= 4.0 * m[0]


# ---- 2: the whole pass against the float64 statement ------------------------------------------------------------------------------------------------
# Largest absolute difference per channel, measured with this very test (it prints them): ALL = every compared pixel, SOLID = those with coverage >= 0.01.
# The ALL figures of the ratio channels -- albedo, normal, depth near 0.9, 1.0 and 1.6 -- are silhouette pixels with a coverage of 1e-6 and less, where the
# weights are known to no digit and a ratio of two such sums says nothing (test_expected_host says why); the B-spline's thin tails make more of them.
MEASURED_ALL = {
    ("c2", 1): (9.00e-01, 9.00e-01, 9.00e-01, 8.50e-06, 9.97e-01, 9.99e-01, 9.93e-01, 1.58e+00),
    ("c2", 2): (9.00e-01, 9.00e-01, 9.00e-01, 3.21e-06, 9.89e-01, 9.58e-01, 9.51e-01, 1.67e+00),
    ("c4_64", 1): (8.00e-01, 8.00e-01, 8.00e-01, 2.47e-06, 1.00e+00, 9.99e-01, 9.82e-01, 1.52e+00),
    ("c4_64", 2): (8.00e-01, 8.00e-01, 8.00e-01, 1.39e-06, 9.76e-01, 9.87e-01, 8.60e-01, 1.51e+00),
    ("c5_64", 1): (9.00e-01, 9.00e-01, 9.00e-01, 2.47e-06, 9.42e-01, 9.94e-01, 9.91e-01, 1.54e+00),
    ("c5_64", 2): (9.00e-01, 9.00e-01, 9.00e-01, 1.36e-06, 9.96e-01, 9.97e-01, 9.86e-01, 1.52e+00),
}
MEASURED_SOLID = {
    ("c2", 1): (5.96e-07, 5.96e-07, 5.96e-07, 8.50e-06, 3.53e-05, 2.90e-05, 3.30e-05, 1.24e-06),
    ("c2", 2): (1.19e-06, 1.19e-06, 1.19e-06, 3.21e-06, 1.60e-05, 1.17e-05, 1.54e-05, 1.80e-06),
    ("c4_64", 1): (2.98e-07, 2.98e-07, 2.98e-07, 2.47e-06, 3.45e-06, 4.25e-06, 3.42e-06, 9.32e-07),
    ("c4_64", 2): (5.96e-07, 5.96e-07, 5.96e-07, 1.39e-06, 1.57e-06, 2.14e-06, 1.41e-06, 8.25e-07),
    ("c5_64", 1): (2.98e-07, 2.98e-07, 2.98e-07, 2.47e-06, 2.49e-06, 3.23e-06, 1.95e-06, 7.41e-07),
    ("c5_64", 2): (5.36e-07, 5.36e-07, 5.36e-07, 1.36e-06, 1.28e-06, 2.05e-06, 1.73e-06, 1.09e-06),
}


@pytest.mark.parametrize("rays", (1, 2))
@pytest.mark.parametrize("name", ("c2", "c4_64", "c5_64"))
def test_host_build_matches_the_float64_statement(name, rays):
    """test_expected_host.test_host_build_matches_the_float64_statement on the cubic field: 64x48; compared are the pixels in which both builds ran the same
    number of steps on every sub-ray (all but 1 % of the covered ones at most); four times the measured largest absolute difference per channel over all of
    them (MEASURED_ALL) and over those with a coverage of 0.01 and more (MEASURED_SOLID)."""
    o = scenes.oracle_scene(name, W, H)
    hc.reset()
    got, m, steps, _, _ = hc.expected_pass(o, rays, 1)
    assert hc.violations()[0] == 0
    ref, m64, steps64 = hc.spec_expected(o, rays, 1)
    assert np.array_equal(m, m64), int((m != m64).sum())
    cut = (steps != steps64).any(axis=2)
    covered = (got[..., 3] > 0) | (ref[..., 3] > 0)
    assert covered.sum() > 500 and not covered.all()
    print("%s rays %d: %d of %d covered pixels left out at the cut, longest sub-ray %d steps" % (name, rays, int(cut.sum()), int(covered.sum()), int(m.max())))
    assert cut.sum() <= 0.01 * covered.sum()
    diff = np.abs(got.astype(np.float64) - ref)
    solid = ~cut & (ref[..., 3] >= 0.01)
    assert solid.sum() > 500
    d_all, d_solid = diff[~cut].max(axis=0), diff[solid].max(axis=0)
    print("all  : (%s)," % ", ".join("%.2e" % x for x in d_all))
    print("solid: (%s)," % ", ".join("%.2e" % x for x in d_solid))
    for c in range(8):
        assert d_all[c] <= 4.0 * MEASURED_ALL[(name, rays)][c], (CH[c], d_all[c])
        assert d_solid[c] <= 4.0 * MEASURED_SOLID[(name, rays)][c], (CH[c], d_solid[c])


# ---- 3: the coverage the path tracer converges to ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spp", (("c2", 4096), ("c4_64", 1024)))
def test_the_cubic_march_gives_the_trackers_coverage_and_the_trilinear_one_does_not(name, spp):
    """The test that shows what the setting is for.  Oracle frame at 64x48 (the scene's own seed), kappa^ its alpha after spp samples; kappa the coverage of
    the host build's 2 x 2 rays.  Over the pixels with kappa < 0.99 (the others are capped by the march's T <= 2^-10 cut, not by the field; at least half of
    the frame must remain): D = mean(kappa^ - kappa), sigma = sqrt(sum kappa (1 - kappa) / spp) / N, z = D / sigma.  |z| <= 4 on the tracker's field,
    z >= 8 on the trilinear one, same frames.  Measured:
                      field 1: kept, D, z           field 0: kept, D, z
      c2    4096 spp  2943  +4.21e-05  +1.04        2944  +4.22e-04  +10.46
      c4_64 1024 spp  2016  +4.85e-05  +0.46        2018  +5.92e-03  +57.98"""
    o = scenes.oracle_scene(name, W, H)
    hat = o.render(spp)[..., 3].copy()
    z = {}
    for field in (1, 0):
        kappa = hc.expected_pass(o, 2, field)[0][..., 3]
        z[field], D, kept = hc.coverage_statistic(hat, kappa, spp)
        print("%s %d spp field %d: kept %d of %d, D %+.3e, z %+.2f" % (name, spp, field, kept, W * H, D, z[field]))
        assert kept >= W * H // 2
    assert abs(z[1]) <= 4.0, z
    assert z[0] >= 8.0, z


# ---- 4: empty space ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c2", "c4_64"))
def test_skipping_by_the_table_of_reach_2_changes_no_bit(name):
    """64x48, 2 x 2 rays, field 1: the frame and the sub-ray records with the table, without it and audited are the same bits; no dropped step has sigma > 0;
    some steps are dropped.  And the test can fail: marching the cubic field with the table of reach 1 drops steps that count."""
    o = scenes.oracle_scene(name, W, H)
    off, on, audit = (hc.expected_pass(o, 2, 1, skip) for skip in (0, 1, 2))
    for got in (on, audit):
        assert _same(got[0], off[0])
        assert np.array_equal(got[1], off[1]) and np.array_equal(got[2], off[2]) and _same(got[3], off[3])
    w0, w1, w2 = off[4], on[4], audit[4]
    assert w2["audit"] == 0, w2
    assert w0["fetched"] == w0["steps"] and w0["reads"] == 0
    assert w1["steps"] == w0["steps"] and w1["rays"] == w0["rays"] and 0 < w1["fetched"] < w1["steps"] and w1["reads"] > 0
    assert {k: w2[k] for k in ("rays", "steps", "fetched", "reads")} == {k: w1[k] for k in ("rays", "steps", "fetched", "reads")}
    wrong = hc.expected_pass(o, 2, 1, 2, reach=1)
    print("%s: %s; with the table of reach 1 the audit finds %d dropped steps with sigma > 0" % (name, w1, wrong[4]["audit"]))
    assert wrong[4]["audit"] > 0
    # field 0 through this harness is the pass as it was: the same bits as the harness that knows no field
    assert _same(hc.expected_pass(o, 2, 0, 1)[0], he.expected_pass(o, 2))


def _blobs_19x9x10():
    z, y, x = _index((10, 9, 19))
    v = np.zeros((10, 9, 19), np.float32)
    for cx, cy, cz, r in ((3.0, 4.0, 5.0, 2.5), (17.5, 1.0, 8.5, 1.5)):
        v += np.maximum(0.0, 1.0 - ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (r * r)).astype(np.float32)
    return v.astype(np.float16)


def _bricks_3x2x1():
    v = np.zeros((8, 16, 24), np.uint8)
    v[3, 2, 1] = 200
    v[7, 15, 23] = 1
    v[0, 9, 9] = 90
    return v


TABLE_GRIDS = {"dense_19x9x10": lambda: encoder_ref.encode_dense_fp16(_blobs_19x9x10()), "bricks_3x2x1": lambda: _brick_grid(_bricks_3x2x1())}


@pytest.mark.parametrize("reach", (1, 2))
@pytest.mark.parametrize("name", sorted(TABLE_GRIDS))
def test_the_host_table_is_the_numpy_statement(name, reach):
    o = _scene_of(TABLE_GRIDS[name]())
    got, want = hc.table(o, reach), hc.spec_table(o.density, reach)
    assert got.shape == want.shape and np.array_equal(got, want), (name, reach, got, want)
    assert got.shape == ((2, 2, 3) if name.startswith("dense") else (1, 2, 3)) and (got == 0).any()
    if reach == 1:
        import hk_expected_skip as hs
        assert np.array_equal(got, hs.table(o))                           # reach 1 is the table as it was


@pytest.mark.parametrize("axis", (0, 1, 2))
@pytest.mark.parametrize("side", (0, 1))
def test_a_voxel_two_away_marks_the_cell_under_reach_2_only(axis, side):
    """24^3 dense voxels, one of them not zero: local index 1 of the cell after the middle one along `axis` (voxel 17), or local index 6 of the cell before it
    (voxel 6).  The middle cell's box grown by one voxel is [7, 16]: clear; grown by two it is [6, 17]: not clear."""
    v = np.zeros((24, 24, 24), np.float16)
    at = [12, 12, 12]
    at[axis] = 17 if side else 6
    v[at[2], at[1], at[0]] = 1.0
    o = _scene_of(encoder_ref.encode_dense_fp16(v))
    t1, t2 = hc.table(o, 1), hc.table(o, 2)
    assert t1[1, 1, 1] == 1 and t2[1, 1, 1] == 0
    assert np.array_equal(t1, hc.spec_table(o.density, 1)) and np.array_equal(t2, hc.spec_table(o.density, 2))
    # and the lookup does read it there: at the middle cell's face towards that voxel the cubic value is positive, the trilinear corners are all +0
    p = np.array([12.25, 12.25, 12.25], np.float32)
    p[axis] = 15.9 if side else 8.1
    assert hc.probe(o, p[None, :])[0, 0] > 0 and hk_features.trilinear(hk_features.decoded_grid(o.density), p[None, :].astype(np.float64))[0] == 0


# ---- 5: under a LUT the tracker's field is the trilinear one ------------------------------------------------------------------------------------------------
def test_under_a_lut_the_setting_changes_no_bit():
    o = scenes.oracle_scene("c3", W, H)
    for skip in (0, 1):
        a, b = hc.expected_pass(o, 2, 0, skip), hc.expected_pass(o, 2, 1, skip)
        assert _same(a[0], b[0]) and a[4] == b[4] and (a[0][..., 3] > 0).any()
    assert _same(hc.expected_pass(o, 2, 1)[0], he.expected_pass(o, 2))
    # ... while without one it does
    o = scenes.oracle_scene("c2", W, H)
    assert not _same(hc.expected_pass(o, 2, 1)[0], hc.expected_pass(o, 2, 0)[0])
