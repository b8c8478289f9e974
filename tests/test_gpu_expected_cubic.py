"""GPU: the expected-value feature pass on the tracker's field (vr_set_int "expected_field" 1; vr_launch.hip features_expected_kernel<false, SKIP, STATS, true>
on volren_amd/csrc/vr_cubic.h, with the clear-distance table of reach 2) bit for bit against the host build of the same headers
(tests/hostkernel/expected_cubic_host.cpp, itself held to float64 statements and to the path tracer's coverage by tests/test_expected_cubic_host.py): on
brick and dense grids, whole and partial tiles, with and without the table, inside the volume, on a cropped view and on a tile subset; its work counts, the
lookup's probe and the table of reach 2; and the setting through the LUT case, the sharded renderer, vr_upsample and its refusals."""
import numpy as np
import pytest

import encoder_ref
import hk_expected_cubic as hc
import scenes
import volren_amd
from hk_common import same as _same
from test_expected_cubic_host import GRIDS, TABLE_GRIDS, _blobs_19x9x10, _bricks_3x2x1, _index, _scene_of

pytestmark = pytest.mark.gpu

VR_ERR = 1
CUBIC = 8                                        # vr_probe.h PROBE_CUBIC


def _features(r, rays, skip=1, field=1):
    r.expected_field, r.expected_skip = field, skip
    r.render_features_expected(rays)
    return r.features()


@pytest.mark.parametrize("name", ("c2", "c4_64", "c5_64"))
def test_the_kernel_matches_the_host_build_bit_for_bit(name):
    """smoke.brick, a dense fp16 grid and brick grids with an emission grid, at 64x48 (whole tiles) with 1 and 2 rays per axis and at 33x17 (partial tiles on
    both edges) with 1, 2 and 4, each with and without the table"""
    r, o = scenes.hip_scene(name, 64, 48), scenes.oracle_scene(name, 64, 48)
    for (w, h), all_rays in (((64, 48), (1, 2)), ((33, 17), (1, 2, 4))):
        r.resize(w, h)
        o.resize(w, h)
        for rays in all_rays:
            host = hc.expected_pass(o, rays, 1)[0]
            for skip in (0, 1):
                assert _same(_features(r, rays, skip), host), (name, w, h, rays, skip)
            assert (host[..., 3] > 0).any() and not (host[..., 3] > 0).all()
    assert not _same(_features(r, 2, 1, 0), _features(r, 2, 1, 1))            # the two fields differ
    r.close()


def _inside(x):
    x.cam_pos, x.cam_dir, x.cam_fov = (0.05, 0.0, -0.1), (0.4, 0.2, 1.0), 80.0


@pytest.mark.parametrize("case", ("inside", "crop"))
def test_a_camera_inside_the_volume_and_the_cropped_view(case):
    """c2 from inside the volume; round 5's cropped view of smoke.brick (tests/golden/host_rows.py R5_SCENES["crop"]); 40x30, 2 x 2 rays, with and without the table"""
    from oracle import binding as ob
    if case == "inside":
        r, o = scenes.hip_scene("c2", 40, 30), scenes.oracle_scene("c2", 40, 30)
        for x in (r, o):
            _inside(x)
    else:
        r, o = scenes.configure_r5(volren_amd.Renderer(40, 30), "crop", False), scenes.configure_r5(ob.OracleRenderer(40, 30), "crop", True)
    host = hc.expected_pass(o, 2, 1)[0]
    for skip in (0, 1):
        assert _same(_features(r, 2, skip), host), (case, skip)
    assert np.isfinite(host).all() and (host[..., 3] > 0).any()
    r.close()


def test_a_tile_subset_marches_the_same_field():
    r, o = scenes.hip_scene("c2", 48, 40), scenes.oracle_scene("c2", 48, 40)      # 3 x 3 tiles, the top row partial
    before = _features(r, 2, 1, 0)                                                # the whole frame on the trilinear field first
    tiles = [1, 3, 7]
    r.set_tiles(tiles)
    after, ref = _features(r, 2, 1, 1), hc.expected_pass(o, 2, 1)[0]
    mask = np.zeros((40, 48), bool)
    for t in tiles:
        ty, tx = divmod(t, 3)
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    assert _same(after[mask], ref[mask]) and (ref[mask][:, 3] > 0).any()
    assert _same(after[~mask], before[~mask]) and not _same(before[mask], ref[mask])
    r.close()


@pytest.mark.parametrize("name", ("c2", "c4_64"))
def test_the_work_counts_are_the_host_builds(name):
    r, o = scenes.hip_scene(name, 64, 48), scenes.oracle_scene(name, 64, 48)
    r.expected_stats = 1
    for rays, skip in ((2, 1), (1, 0)):
        feat = _features(r, rays, skip)
        got, host = r.expected_stats(), hc.expected_pass(o, rays, 1, skip)
        assert _same(feat, host[0])
        assert got == {k: host[4][k] for k in ("rays", "steps", "fetched", "reads")}, (name, rays, skip, got, host[4])
        if skip:
            assert got["fetched"] < got["steps"] and got["reads"] > 0
        else:
            assert got["fetched"] == got["steps"] and got["reads"] == 0
    r.close()


def _tiny_pair(name):
    """the ramp grid `name` of test_expected_cubic_host.GRIDS on the device and in the oracle"""
    G = GRIDS[name]
    z, y, x = _index(G["shape"])
    b, sx, sy, sz = G["ramp"]
    vox = b + sx * x + sy * y + sz * z
    r = volren_amd.Renderer(16, 16)
    r.load_envmap(scenes.HDR)
    if name.startswith("dense"):
        r.set_volume_dense_f16(vox.astype(np.float16))
        return r, _scene_of(encoder_ref.encode_dense_fp16(vox.astype(np.float16)))
    a = hc.brick_arrays(vox)
    r.set_volume_brick(a["transform"], a["n_bricks"], a["min_maj"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"], commit=True)
    return r, _scene_of(hc.oracle_brick_grid(a))


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_the_probe_is_the_host_lookup_bit_for_bit(name):
    """vr_probe PROBE_CUBIC over hk_expected_cubic.catalogue -- t = 0, the float below 1, brick faces, borders from both sides, negative coordinates, -0, a
    denormal, NaN, +-inf, +-2^30 -- in the compiled-in form of the grid and in the run-time form the kernel uses"""
    r, o = _tiny_pair(name)
    nz, ny, nx = GRIDS[name]["shape"]
    pts = hc.catalogue((nx, ny, nz))
    items = np.zeros((len(pts), 4), np.uint32)
    items[:, 1:] = pts.view(np.uint32)
    host = hc.probe(o, pts)
    for form in ((1, 2) if name.startswith("dense") else (0, 2)):
        got = r.probe(CUBIC, form, items)
        assert got.shape == host.shape and _same(got, host), (name, form, int((got.view(np.uint32) != host.view(np.uint32)).any(axis=1).sum()))
    with pytest.raises(volren_amd.VolrenError, match="DENSE"):
        r.probe(CUBIC, 0 if name.startswith("dense") else 1, items[:4])
    with pytest.raises(volren_amd.VolrenError, match="form out of range"):
        r.probe(CUBIC, 3, items[:4])
    r.close()


@pytest.mark.parametrize("name", sorted(TABLE_GRIDS))
def test_the_table_of_reach_2_is_the_numpy_statement(name):
    """a dense 19 x 9 x 10 grid and 3 x 2 x 1 bricks: vr_expected_clear_table returns the table the current setting marches with"""
    r = volren_amd.Renderer(16, 16)
    r.load_envmap(scenes.HDR)
    if name.startswith("dense"):
        vox = _blobs_19x9x10()
        r.set_volume_dense_f16(vox)
        o = _scene_of(encoder_ref.encode_dense_fp16(vox))
    else:
        a = hc.brick_arrays(_bricks_3x2x1())
        r.set_volume_brick(a["transform"], a["n_bricks"], a["min_maj"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"], commit=True)
        o = _scene_of(hc.oracle_brick_grid(a))
    want = {reach: hc.spec_table(o.density, reach) for reach in (1, 2)}
    assert not np.array_equal(want[1], want[2])
    for field in (1, 0, 1):                                                  # each table is built once and found again
        r.expected_field = field
        got = r.expected_clear_table()
        assert got.shape == want[1 + field].shape and np.array_equal(got, want[1 + field]), (name, field)
        assert np.array_equal(got, hc.table(o, 1 + field))
    r.close()


def test_under_a_lut_the_setting_changes_no_bit():
    r = scenes.hip_scene("c3", 50, 38)
    for skip in (0, 1):
        assert _same(_features(r, 2, skip, 0), _features(r, 2, skip, 1))
    r.expected_field = 1
    t1 = r.expected_clear_table()
    r.expected_field = 0
    assert np.array_equal(t1, r.expected_clear_table()) and (t1 > 0).any()     # and marches with the table of reach 1
    r.close()


def test_two_logical_shards_equal_the_single_device():
    one = scenes.hip_scene("c2", 72, 56)
    want = _features(one, 2)
    s = volren_amd.ShardedRenderer(72, 56, [0, 0])
    s.each(lambda p: scenes.configure(p, "c2", False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    s.render(2)                                                    # the gather of the guides wants a frame with its moments
    assert s.expected_field == 0
    s.expected_field = 1
    assert s.expected_field == 1 and all(p.expected_field == 1 for p in s.parts)
    s.render_features_expected(2)
    assert _same(s.features(), want)
    s.expected_field = 0
    s.render_features_expected(2)
    assert _same(s.features(), _features(one, 2, 1, 0)) and not _same(s.features(), want)
    s.close()
    one.close()


def test_upsample_marches_the_hi_pass_on_the_same_field():
    """c2, lo 24x19, f = 3, 2 x 2 rays: vr_upsampled_features after vr_upsample against a renderer of 72x57 with the same setting"""
    big = scenes.hip_scene("c2", 72, 57)
    want = {field: _features(big, 2, 1, field) for field in (0, 1)}
    r = scenes.hip_scene("c2", 24, 19)
    r.variance = 1
    r.denoise_layers = 1
    for field in (1, 0):
        r.expected_field = field
        r.reset()
        r.render(4)
        r.render_features_expected(2)
        r.denoise()
        r.upsample(3, 2)
        assert _same(r.upsampled_features(), want[field]), field
    assert not _same(want[0], want[1])
    big.close()
    r.close()


def test_the_setting_its_default_and_its_refusals():
    lib = volren_amd.load()
    r = scenes.hip_scene("c2", 16, 16)
    assert r.expected_field == 0 and r.get_int("expected_field") == 0
    default = _features(r, 2, 1, 0)
    fresh = scenes.hip_scene("c2", 16, 16)
    fresh.render_features_expected(2)
    assert _same(fresh.features(), default)                                   # the default is the trilinear march
    fresh.close()
    for v in (1, 0):
        r.expected_field = v
        assert r.get_int("expected_field") == v
        for bad in (-1, 2, 2 ** 31 - 1):
            assert lib.vr_set_int(r._h, b"expected_field", bad) == VR_ERR and b"expected_field: 0 (march the trilinear field) or 1" in lib.vr_last_error()
            assert r.get_int("expected_field") == v
    r.close()
