"""GPU: denoiser data.  The feature pass (vr_render_features) bit for bit against the host-compiled lane code (tests/hostkernel/features_host.cpp,
itself held to the oracle's orc_sample_volume by tests/test_features_host.py); the per-pixel variance (vr_set_int "variance", vr_variance) against
the oracle's per-sample radiances; the Python and volpy interfaces."""
import ctypes as C

import numpy as np
import pytest

import hk_features
import scenes
import volren_amd

pytestmark = pytest.mark.gpu

FEATURE_SCENES = ("c1", "c3", "c4_64", "c5_64")


def _pair(name, w, h):
    return scenes.hip_scene(name, w, h), scenes.oracle_scene(name, w, h)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", FEATURE_SCENES)
@pytest.mark.parametrize("spp", (1, 7))
def test_features_match_the_host_lane_code(name, spp):
    r, o = _pair(name, 32, 24)
    r.render_features(spp)
    got = r.features()
    ref = hk_features.feature_pass(o, spp)
    assert np.array_equal(_bits(got), _bits(ref)), (name, spp, int((_bits(got) != _bits(ref)).any(axis=2).sum()))
    assert (got[..., 3] > 0).any()


def test_features_on_a_ragged_frame():
    r, o = _pair("c1", 50, 37)
    r.render_features(3)
    assert np.array_equal(_bits(r.features()), _bits(hk_features.feature_pass(o, 3)))


def test_features_with_a_clip_box():
    r, o = _pair("c3", 40, 30)
    for x in (r, o):
        x.vol_clip_min = (0.1, 0.2, 0.0)
        x.vol_clip_max = (0.8, 0.9, 0.7)
    r.render_features(4)
    assert np.array_equal(_bits(r.features()), _bits(hk_features.feature_pass(o, 4)))


def test_features_with_a_tile_subset_leave_other_pixels_alone():
    r, o = _pair("c1", 48, 40)                  # 3 x 3 tiles, the top row ragged
    r.render_features(1)
    before = r.features()
    tiles = [1, 3, 7]
    r.set_tiles(tiles)
    r.render_features(5)
    after = r.features()
    ref = hk_features.feature_pass(o, 5)
    mask = np.zeros((40, 48), bool)
    for t in tiles:
        ty, tx = divmod(t, 3)
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    assert np.array_equal(_bits(after[mask]), _bits(ref[mask]))
    assert np.array_equal(_bits(after[~mask]), _bits(before[~mask]))


def test_features_before_any_feature_pass_fail():
    r = scenes.hip_scene("c1", 16, 16)
    with pytest.raises(volren_amd.VolrenError):
        r.features()
    r.render_features(1)
    r.features()
    r.resize(24, 16)
    with pytest.raises(volren_amd.VolrenError, match="render_features"):
        r.features()


def test_far_camera_is_bounded_and_reported():
    """t + dt rounds back to t (the reference's tracker never ends there): stalled segments end without a collision; a pixel whose segment
    exceeds the step budget stops and vr_synchronize reports it.  Same outcome as the host build, bit for bit; the renderer works on afterwards."""
    for k, fails in ((1e7, False), (1e5, True)):
        r, o = _pair("c1", 8, 8)
        near = np.asarray(r.cam_pos, np.float32)
        for x in (r, o):
            x.cam_pos = tuple(float(v) * k for v in near)
            x.cam_fov = 70.0 / k
        ref, lost = hk_features.feature_pass(o, 2, with_lost=True)
        assert (lost > 0) == fails
        if fails:
            with pytest.raises(volren_amd.VolrenError, match="feature pass"):
                r.render_features(2)
        else:
            r.render_features(2)
        assert np.array_equal(_bits(r.features()), _bits(ref)), k
        for x in (r, o):                     # the status was read and cleared: a pass of the near camera reports nothing
            x.cam_pos = tuple(float(v) for v in near)
            x.cam_fov = 40.0
        r.render_features(2)
        assert np.array_equal(_bits(r.features()), _bits(hk_features.feature_pass(o, 2)))


# ---- variance ----------------------------------------------------------------------------------------------------------------------------------
def _oracle_radiance(o, spp, integrator=0):
    o.integrator = integrator
    L = np.zeros((spp, o.h, o.w, 4), np.float32)
    for y in range(o.h):
        for x in range(o.w):
            for k in range(spp):
                L[k, y, x] = o.trace_pixel_sample(x, y, k + 1)
    return L


def _replay(L):
    """The two mix_ lines of the accumulation pass in float32, samples in order; -> (mean, S)."""
    mu = np.zeros(L.shape[1:], np.float32)
    S = np.zeros(L.shape[1:], np.float32)
    one = np.float32(1.0)
    for k in range(L.shape[0]):
        a = one / np.float32(k + 1)
        x = np.where(np.isfinite(L[k]), L[k], np.float32(0)).astype(np.float32)
        mu1 = (mu * (one - a) + x * a).astype(np.float32)
        S = (S * (one - a) + ((x - mu) * (x - mu1)).astype(np.float32) * a).astype(np.float32)
        mu = mu1
    return mu, S


def _ulps(a, b):
    ia = _bits(a).astype(np.int64)
    ib = _bits(b).astype(np.int64)
    ia = np.where(ia >= 2 ** 31, 2 ** 31 - ia, ia)
    ib = np.where(ib >= 2 ** 31, 2 ** 31 - ib, ib)
    return np.abs(ia - ib)


def _check_variance(r, L):
    n = L.shape[0]
    mu, S = _replay(L)
    var = r.variance()
    expect = (S * (np.float32(n) / np.float32(n - 1))).astype(np.float32)
    assert _ulps(var, expect).max() <= 1, int(_ulps(var, expect).max())
    two = np.where(np.isfinite(L), L, 0).astype(np.float64).var(axis=0, ddof=1)
    big = two > 1e-6
    assert big.sum() > 50
    assert (np.abs(var[big] - two[big]) / two[big]).max() <= 1e-4
    return mu


@pytest.mark.parametrize("name", ("c1", "c3"))
def test_variance_matches_the_oracle_samples(name):
    r, o = _pair(name, 64, 48)
    L = _oracle_radiance(o, 16)
    r.variance = 1
    r.render(16)
    mu = _check_variance(r, L)
    assert np.array_equal(_bits(r.framebuffer()), _bits(mu))


@pytest.mark.parametrize("name,integrator", (("c3", 2), ("c1", 3)))
def test_variance_of_the_other_integrators(name, integrator):
    r, o = _pair(name, 32, 24)
    L = _oracle_radiance(o, 8, integrator)
    r.integrator = integrator
    r.variance = 1
    r.render(8)
    _check_variance(r, L)


def test_variance_leaves_the_colour_alone_and_does_not_depend_on_the_launch_split():
    r = scenes.hip_scene("c1", 64, 48)
    r.render(12)
    plain = r.framebuffer()
    r.reset()
    r.variance = 1
    r.render(12)
    assert np.array_equal(_bits(r.framebuffer()), _bits(plain))
    ref = r.variance()
    r.reset()
    while r.sample < 12:                     # the reference's loop (coalesced trace() calls)
        r.trace()
    assert np.array_equal(_bits(r.variance()), _bits(ref))
    r.reset()
    r.coalesce_trace = 0
    for _ in range(12):                      # one launch per sample: the moments reloaded 11 times
        r.trace()
    assert np.array_equal(_bits(r.variance()), _bits(ref))
    assert np.array_equal(_bits(r.framebuffer()), _bits(plain))


def test_variance_over_several_sub_launches():
    r = scenes.hip_scene("c1", 256, 256)
    r.variance = 1
    r.render(40)
    ref, fb = r.variance(), r.framebuffer()
    r.sample_pool_mb = 16                    # 1 MiB per sample of this frame: three sub-launches
    r.reset()
    r.render(40)
    assert r.last_launches >= 3
    assert np.array_equal(_bits(r.variance()), _bits(ref))
    assert np.array_equal(_bits(r.framebuffer()), _bits(fb))


def test_variance_switched_on_mid_frame_is_refused_until_reset():
    r = scenes.hip_scene("c1", 32, 24)
    r.render(4)
    r.variance = 1
    r.render(4)
    with pytest.raises(volren_amd.VolrenError, match="mid-frame"):
        r.variance()
    r.reset()
    r.render(8)
    v = r.variance()
    assert np.isfinite(v).all() and (v > 0).any()
    r.variance = 0
    r.render(2)                              # samples 9..10 without moments
    with pytest.raises(volren_amd.VolrenError):
        r.variance()
    r.reset()
    r.variance = 1
    r.render(1)
    assert np.all(r.variance() == 0)         # n = 1


# ---- Python and volpy --------------------------------------------------------------------------------------------------------------------------
def test_python_and_volpy_shapes_and_row_order():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.cam_fov = 40.0
    vr.variance = 1
    assert vr.variance == 1
    vr.render(6)
    vr.render_features(6)
    r = vr._r
    L = r._L
    raw_f = np.empty(24 * 40 * 8, np.float32)
    raw_v = np.empty(24 * 40 * 4, np.float32)
    assert L.vr_features(r._h, raw_f.ctypes.data) == 0 and L.vr_variance(r._h, raw_v.ctypes.data) == 0
    f, v = r.features(), r.variance()
    assert f.shape == (24, 40, 8) and v.shape == (24, 40, 4)
    assert np.array_equal(f.reshape(-1), raw_f) and np.array_equal(v.reshape(-1), raw_v)      # row 0 = bottom, like framebuffer()
    fd, vd = vr.feature_data(), vr.variance_data()
    assert fd.shape == (40, 24, 8) and vd.shape == (40, 24, 3) and vr.fbo_data().shape == (40, 24, 3)
    assert np.array_equal(fd.reshape(-1), raw_f) and np.array_equal(vd.reshape(-1), v[..., :3].reshape(-1))


def test_volpy_script_in_the_datagen_denoise_style(tmp_path):
    """The call protocol of scripts/datagen_denoise.py (noisy / clean colour pairs) with the auxiliary buffers added."""
    import volren_amd.volpy as volpy
    renderer = volpy.Renderer(32, 32)
    renderer.volume = volpy.Volume(scenes.SMOKE)
    renderer.environment = volpy.Environment(scenes.HDR)
    renderer.scale_and_move_to_unit_cube()
    renderer.commit()
    renderer.variance = 1
    out = {}
    for i, spp in enumerate((4, 16)):
        renderer.seed = 42 + i
        renderer.render(spp)
        renderer.render_features(spp)
        out[spp] = dict(color=np.flip(np.array(renderer.fbo_data()), axis=0), features=np.flip(np.array(renderer.feature_data()), axis=0),
                        variance=np.flip(np.array(renderer.variance_data()), axis=0))
        np.save(tmp_path / ("features_%d.npy" % spp), out[spp]["features"])
    for spp, d in out.items():
        assert d["color"].shape == (32, 32, 3) and d["features"].shape == (32, 32, 8) and d["variance"].shape == (32, 32, 3)
        assert np.isfinite(d["features"]).all() and np.isfinite(d["variance"]).all()
        cov = d["features"][..., 3]
        assert ((cov >= 0) & (cov <= 1)).all() and cov.max() > 0
