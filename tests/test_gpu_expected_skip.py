"""GPU: empty-space skipping in the expected-value feature pass (vr_set_int "expected_skip"; vr_launch.hip features_expected_kernel with the clear-distance
table of vr_setup.hip clear_mark_kernel / clear_axis_kernel).  The frame with the table, the frame without it and the host build of the same header
(tests/hostkernel/expected_host.cpp) are the same bits; the device's table is the host's (tests/hostkernel/expected_skip_host.cpp, itself held to a numpy
statement by tests/test_expected_skip_host.py) byte for byte; the device's work counters are the host's; a table never outlives its grid.
Frames of 72x56: partial 16x16 tiles on both edges."""
import numpy as np
import pytest

import hk_expected as he
import hk_expected_skip as hs
import scenes
import volren_amd
from hk_common import same as _same
from test_expected_skip_capi import check_settings
from test_expected_skip_host import _blobs_60x44x52

pytestmark = pytest.mark.gpu

W, H = 72, 56
SCENES = ("c1", "c3", "c4_64", "c5_64")        # smoke.brick, + lut.txt (decoded float atlas), a 64^3 dense fp16 grid, a 64^3 sparse pair with an emission grid


def _features(r, rays, skip):
    r.expected_skip = skip
    r.render_features_expected(rays)
    return r.features()


@pytest.mark.parametrize("name", SCENES)
def test_skip_on_skip_off_and_the_host_build_are_the_same_bits(name):
    r, o = scenes.hip_scene(name, W, H), scenes.oracle_scene(name, W, H)
    for rays in (1, 3):
        off, on, host = _features(r, rays, 0), _features(r, rays, 1), he.expected_pass(o, rays)
        assert _same(on, off) and _same(on, host), (name, rays)
        assert (on[..., 3] > 0).any() and not (on[..., 3] > 0).all()
    r.close()


def _dense_pair():
    from oracle import binding as ob
    import encoder_ref
    vox = _blobs_60x44x52()
    r = volren_amd.Renderer(16, 16)
    r.set_volume_dense_f16(vox)
    o = ob.OracleRenderer(16, 16)
    o.set_volume(encoder_ref.encode_dense_fp16(vox))
    return r, o


@pytest.mark.parametrize("name", SCENES + ("dense_60x44x52",))
def test_the_device_table_is_the_host_table(name):
    r, o = _dense_pair() if name == "dense_60x44x52" else (scenes.hip_scene(name, 16, 16), scenes.oracle_scene(name, 16, 16))
    got, want = r.expected_clear_table(), hs.table(o)
    assert got.shape == want.shape and np.array_equal(got, want), (name, got.shape, want.shape, int((got != want).sum()) if got.shape == want.shape else -1)
    assert (got == 0).any() and (got > 0).any()
    assert np.array_equal(r.expected_clear_table(), want)                      # the second call finds the table
    r.close()


@pytest.mark.parametrize("name", SCENES)
def test_the_counters_are_the_host_builds(name):
    """the same float32 arithmetic on both sides: sub-rays marched, steps reached, steps that fetched and table reads agree exactly; without the table every
    step reached fetches and the table is not read; a pass that did not count has no counters"""
    r, o = scenes.hip_scene(name, W, H), scenes.oracle_scene(name, W, H)
    r.render_features_expected(2)
    with pytest.raises(volren_amd.VolrenError, match="expected_stats"):
        r.expected_stats()
    r.expected_stats = 1
    for rays, skip in ((1, 1), (3, 1), (2, 0)):
        feat = _features(r, rays, skip)
        got, host = r.expected_stats(), hs.expected_pass(o, rays, skip)
        assert _same(feat, host[0])
        assert got == {k: host[4][k] for k in ("rays", "steps", "fetched", "reads")}, (name, rays, skip, got, host[4])
        if skip:
            assert got["fetched"] < got["steps"] and got["reads"] > 0
        else:
            assert got["fetched"] == got["steps"] and got["reads"] == 0
    r.expected_stats = 0
    r.render_features_expected(2)
    with pytest.raises(volren_amd.VolrenError, match="expected_stats"):
        r.expected_stats()
    r.close()


def _blob(n, cx, cy, cz, rad):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.maximum(0.0, 1.0 - ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (rad * rad)).astype(np.float32)


def _animation(frames, counter, skip, w=W, h=H):
    r = volren_amd.Renderer(w, h)
    r.load_envmap(scenes.HDR)
    r.set_volume_dense(frames[0], commit=False)
    for f in frames[1:]:
        r.volume_add_grid_frame(f)
    r.commit()
    r.density_scale, r.cam_fov, r.grid_frame_counter, r.expected_skip = 40.0, 40.0, counter, skip
    return r


def test_a_table_never_outlives_its_grid():
    """two frames of 40^3 voxels with their smoke in opposite corners.  After grid_frame_counter moves, and after frame 1 is replaced and committed, the pass is
    that of a fresh renderer on the same frames that marches every step: a table left over from another grid would drop steps that count"""
    a, b, c = _blob(40, 9.0, 9.0, 9.0, 7.0), _blob(40, 30.0, 30.0, 30.0, 7.0), _blob(40, 30.0, 9.0, 20.0, 7.0)
    r = _animation([a, b], 0, 1)
    first = _features(r, 2, 1)
    r.grid_frame_counter = 1
    second = _features(r, 2, 1)
    r.volume_update_grid_frame(1, c)
    r.commit()
    third = _features(r, 2, 1)
    r.grid_frame_counter = 0
    again = _features(r, 2, 1)
    for got, frames, counter in ((first, [a, b], 0), (second, [a, b], 1), (third, [a, c], 1), (again, [a, c], 0)):
        fresh = _animation(frames, counter, 0)
        want = _features(fresh, 2, 0)
        fresh.close()
        assert _same(got, want) and (got[..., 3] > 0).sum() > 50
    assert not _same(first, second) and not _same(second, third) and _same(first, again)
    r.close()


def test_two_logical_shards_equal_the_single_device():
    one = scenes.hip_scene("c1", W, H)
    want = _features(one, 2, 0)
    s = volren_amd.ShardedRenderer(W, H, [0, 0])
    s.each(lambda p: scenes.configure(p, "c1", False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    s.render(2)                                                    # the gather of the guides wants a frame with its moments
    for skip in (1, 0):
        s.expected_skip = skip
        assert s.expected_skip == skip and all(p.expected_skip == skip for p in s.parts)
        s.render_features_expected(2)
        assert _same(s.features(), want), skip
    s.close()
    one.close()


def test_switching_the_setting_within_one_renderer():
    r = scenes.hip_scene("c3", W, H)
    check_settings(r)
    a, b, c = _features(r, 2, 0), _features(r, 2, 1), _features(r, 2, 0)
    assert _same(a, b) and _same(b, c) and (a[..., 3] > 0).any()
    r.close()
