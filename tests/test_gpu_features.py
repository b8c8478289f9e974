"""GPU: denoiser data.  The feature pass (vr_render_features) bit for bit against the host-compiled lane code (tests/hostkernel/features_host.cpp,
itself held to the oracle's orc_sample_volume by tests/test_features_host.py); the per-pixel variance (vr_set_int "variance", vr_variance) against
the oracle's per-sample radiances; the Python and volpy interfaces."""
import ctypes as C

import numpy as np
import pytest

from hk_common import bits as _bits
import hk_features
import scenes
import volren_amd

pytestmark = pytest.mark.gpu

FEATURE_SCENES = ("c1", "c3", "c4_64", "c5_64")


def _pair(name, w, h):
    return scenes.hip_scene(name, w, h), scenes.oracle_scene(name, w, h)


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


# ---- the feature pass on every grid form, majorant layout, full-size grid and state change ------------------------------------------------------
from test_gpu_parity import _hip_emission_scene, _oracle_emission_scene          # noqa: E402  (the emission scene of the parity tests)


def _same_features(r, o, spp, what, ref=None):
    """r.render_features(spp) bit for bit the host pass of the oracle scene o (or `ref`), and not a trivial buffer"""
    r.render_features(spp)
    got = r.features()
    if ref is None:
        ref = hk_features.feature_pass(o, spp)
    bad = (_bits(got) != _bits(ref)).any(axis=2)
    assert not bad.any(), (what, int(bad.sum()))
    assert (got[..., 3] > 0).any() and (np.abs(got[..., 4:7]).sum(axis=2) > 0).any(), what
    return ref


@pytest.mark.parametrize("lut", (False, True))
def test_features_with_a_blocked_majorant_table(lut):
    r, o = _hip_emission_scene(40, 30), _oracle_emission_scene(40, 30)
    if lut:
        r.load_transferfunc(scenes.LUT)
        o.load_transferfunc(scenes.LUT)
    ref = hk_features.feature_pass(o, 3)
    for layout in (1, 0, 1, -1):
        r.majorant_layout = layout
        assert r.majorant_blocked == (1 if layout == 1 else 0)
        _same_features(r, o, 3, ("emission scene, majorant layout", layout, lut), ref)
    c, co = _pair("c5_64", 40, 30)
    c.majorant_layout = 1
    assert c.majorant_blocked == 1
    _same_features(c, co, 3, "c5:64, blocked majorant table")


def _other_layout_pair(w, h):
    """test_gpu_parity.test_emission_grid_with_a_different_brick_layout's scene: a 40^3 temperature grid scaled 1.8x over a 72^3 density grid
    (8^3 against 16^3 bricks, no paired atlas)"""
    from oracle import binding as ob
    import encoder_ref
    dens = scenes.synthetic_density(72, blobs=12)
    temp = np.clip(scenes.synthetic_density(40, seed=99) * 0.2, 0, None).astype(np.float32)
    t_temp = np.diag([1.8, 1.8, 1.8, 1.0]).astype(np.float32).reshape(16)
    ad, at = encoder_ref.encode_arrays(dens), encoder_ref.encode_arrays(temp, t_temp)
    r = volren_amd.Renderer(w, h)
    r.load_envmap(scenes.HDR)
    r.set_volume_brick(ad["transform"], ad["n_bricks"], ad["min_maj"], ad["indirection"], ad["rng"], ad["atlas_dim"], ad["atlas"], ad["mips"], commit=False)
    r.set_volume_brick(at["transform"], at["n_bricks"], at["min_maj"], at["indirection"], at["rng"], at["atlas_dim"], at["atlas"], at["mips"], name="temperature", commit=True)
    o = ob.OracleRenderer(w, h)
    o.load_envmap(scenes.HDR)
    o.set_volume(encoder_ref.encode(dens), emission=encoder_ref.encode(temp, t_temp), majorant_emission=at["min_maj"][1])
    for x in (r, o):
        x.cam_fov, x.bounces, x.albedo, x.emission_scale = 40.0, 8, (0.7, 0.8, 0.9), 50.0
    return r, o


def _dense_with_emission_pair(w, h):
    """test_gpu_parity.test_dense_fp16_density_with_emission_grid's scene: dense fp16 density + brick temperature grid (run-time variant)"""
    from oracle import binding as ob
    import encoder_ref
    n = 48
    dens = scenes.synthetic_density(n)
    temp = np.clip(dens * 0.15 + 0.05 * scenes.synthetic_density(n, seed=5), 0, None).astype(np.float32)
    r = volren_amd.Renderer(w, h)
    r.load_envmap(scenes.HDR)
    r.set_volume_dense_f16(dens, commit=False)
    r.set_volume_dense(temp, name="temperature", commit=True)
    o = ob.OracleRenderer(w, h)
    o.load_envmap(scenes.HDR)
    gt = encoder_ref.encode(temp)
    gt.extent = (n, n, n)
    gt.c.extent[:] = gt.extent
    o.set_volume(encoder_ref.encode_dense_fp16(dens), emission=gt, majorant_emission=float(temp.max()))
    for x in (r, o):
        x.cam_fov, x.bounces, x.albedo, x.phase, x.density_scale, x.emission_scale = 40.0, 12, (0.7, 0.8, 0.9), 0.2, 60.0, 80.0
    return r, o


def test_features_of_an_emission_grid_with_another_brick_layout():
    r, o = _other_layout_pair(48, 36)
    _same_features(r, o, 4, "emission grid of another layout")


def test_features_of_a_dense_density_with_a_brick_emission_grid():
    r, o = _dense_with_emission_pair(48, 36)
    assert r.kernel_variant == 3
    _same_features(r, o, 4, "dense fp16 density + emission grid")


def test_features_of_the_second_animation_frame_without_a_render_between(tmp_path):
    """test_gpu_parity.test_volume_animation_folder's two frames: a feature pass of frame 0, grid_frame_counter = 1, a feature pass of frame 1 with
    no render() in between"""
    from oracle import binding as ob
    lib = volren_amd.load()
    for i, s in enumerate((5, 6)):
        f = scenes.synthetic_density(40, seed=s)
        assert lib.vr_write_brick_from_dense(f.ctypes.data, 40, 40, 40, None, str(tmp_path / ("f%03d.brick" % i)).encode()) == 0
    r = volren_amd.Renderer(40, 40)
    r.load_envmap(scenes.HDR)
    r.load_volume(tmp_path)
    assert r.n_grid_frames == 2
    r.cam_fov, r.bounces = 40.0, 6
    refs = []
    for i in range(2):
        o = ob.OracleRenderer(40, 40)
        o.load_envmap(scenes.HDR)
        o.load_volume(str(tmp_path / ("f%03d.brick" % i)))
        o.cam_fov, o.bounces = 40.0, 6
        refs.append(hk_features.feature_pass(o, 3))
    assert not np.array_equal(refs[0], refs[1])
    for i in (0, 1, 0):
        r.grid_frame_counter = i
        _same_features(r, None, 3, ("animation frame", i), refs[i])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ("c4", "c5full", "c5cloud"))
def test_features_on_the_full_size_grids(name):
    """c4 (512^3 dense fp16), c5full (1024^3 bricks, 2^21-entry brick tables) and c5cloud (1024^3, the blocked majorant table that commit() picks)"""
    r, o = _pair(name, 96, 64)
    if name == "c5cloud":
        assert r.majorant_blocked == 1
    _same_features(r, o, 2, name)


@pytest.mark.parametrize("name", ("c2", "c1_inside"))
def test_features_of_the_bench_scene_and_a_camera_inside_the_box(name):
    r, o = _pair(name[:2], 48, 36)
    if name == "c1_inside":                 # test_gpu_parity's camera_inside: first scatters close to the camera
        for x in (r, o):
            x.cam_pos, x.cam_dir, x.cam_fov = (0.05, 0.0, -0.1), (0.4, 0.2, 1.0), 80.0
    _same_features(r, o, 4, name)
    if name == "c1_inside":
        got = r.features()
        hit = got[..., 3] > 0
        assert got[hit, 7].min() < 0.05, got[hit, 7].min()


def test_features_follow_state_changes_without_a_render_between():
    r, o = _pair("c3", 40, 30)
    _same_features(r, o, 3, "c3")
    for x in (r, o):
        x.density_scale = 60.0
    _same_features(r, o, 3, "density_scale")
    rng = np.random.default_rng(3)
    lut = rng.random((64, 4)).astype(np.float32)
    lut[:8, 3] = 0.0
    for x in (r, o):                        # a new LUT comes with the default window on the renderer (the window belongs to the LUT)
        x.set_transferfunc(lut)
    _same_features(r, o, 3, "replaced LUT")
    for x in (r, o):
        x.tf_window_left, x.tf_window_width = 0.05, 0.4
    _same_features(r, o, 3, "tf window")


def test_features_do_not_depend_on_the_switches_of_the_colour_path():
    """fast_math, the integrator, the scheduler's thresholds and trace() calls still pending: the same features bit for bit"""
    r, o = _pair("c1", 40, 30)
    ref = _same_features(r, o, 3, "c1")
    r.fast_math = 1
    _same_features(r, o, 3, "fast_math", ref)
    r.fast_math = 0
    for it in (1, 3):
        r.integrator = it
        _same_features(r, o, 3, ("integrator", it), ref)
    r.integrator = 0
    for thr in ([8, 0, 8, 40, 8, 8, 8, 0], [64, 0, 64, 63, 64, 64, 64, 0]):
        r.set_sched(thr)
        _same_features(r, o, 3, ("scheduler", thr), ref)
    r.set_sched([64, 0, 56, 0, 60, 60, 64, 0])
    r.reset()
    for _ in range(3):
        r.trace()
    _same_features(r, o, 3, "trace() pending", ref)
    c, co = _pair("c3", 40, 30)
    cref = _same_features(c, co, 3, "c3")
    c.integrator = 2
    _same_features(c, co, 3, "c3, integrator 2", cref)


def test_features_of_a_1080p_frame():
    """1920 x 1080: 120 x 68 tiles, the top row 8 pixels high"""
    r, o = _pair("c4_64", 1920, 1080)
    _same_features(r, o, 1, "c4:64 at 1920x1080")


# ---- variance on every kernel, at high sample counts, on tile subsets and in the tolerance mode --------------------------------------------------
@pytest.mark.parametrize("name", ("c2", "c4_64", "c5_64", "emission_blocked", "c1_integrator1"))
def test_variance_on_the_other_kernels(name):
    if name == "emission_blocked":
        r, o = _hip_emission_scene(24, 16), _oracle_emission_scene(24, 16)
        r.majorant_layout = 1
        assert r.majorant_blocked == 1
    else:
        r, o = _pair(name[:2] if name.startswith("c1") else name, 24, 16)
    integrator = 1 if name == "c1_integrator1" else 0
    r.integrator = integrator
    L = _oracle_radiance(o, 8, integrator)
    r.variance = 1
    r.render(8)
    mu = _check_variance(r, L)
    assert np.array_equal(_bits(r.framebuffer()), _bits(mu)) and (r.variance() > 0).any()


def _replay_f64_error(L, var):
    """max relative difference of the float32 variance to a float64 two-pass variance, over the entries above 1e-6"""
    two = np.where(np.isfinite(L), L, 0).astype(np.float64).var(axis=0, ddof=1)
    big = two > 1e-6
    assert big.sum() > 50
    return float((np.abs(var[big] - two[big]) / two[big]).max())


@pytest.mark.parametrize("name,spp,bound", (("c1", 1024, 5e-5), ("c2", 256, 5e-5)))
def test_variance_at_high_sample_counts(name, spp, bound):
    """1024 spp of c1 at 24x16, 256 spp of c2 at 16x12: the device within 1 ulp of the float32 replay, and the replay within `bound` (relative, on
    the entries above 1e-6) of a float64 two-pass variance.  The replay runs on the CPU; measured there: 1.10e-5 for c1 at 1024 spp, 6.9e-6 for
    c2 at 256 spp."""
    w, h = (24, 16) if name == "c1" else (16, 12)
    r, o = _pair(name, w, h)
    L = _oracle_radiance(o, spp)
    mu, S = _replay(L)
    expect = (S * (np.float32(spp) / np.float32(spp - 1))).astype(np.float32)
    r.variance = 1
    r.render(spp)
    var = r.variance()
    assert (var >= 0).all() and (var > 0).any()
    assert _ulps(var, expect).max() <= 1, int(_ulps(var, expect).max())
    assert _replay_f64_error(L, expect) <= bound
    assert np.array_equal(_bits(r.framebuffer()), _bits(mu))


def test_variance_of_constant_radiance_is_tiny_and_not_negative():
    """c2 under a 1x1 white environment at 1024 spp: a sample that misses the volume has radiance 1 exactly.  Pixels whose samples all missed
    get 0 <= var <= 2e-12 (the running float32 form need not give exactly 0; on this frame it does), and every variance is >= 0"""
    spp = 1024
    r, o = _pair("c2", 16, 12)
    for x in (r, o):
        x.set_envmap(np.ones((1, 1, 3), np.float32))
    L = _oracle_radiance(o, spp)
    miss = (L[..., :3] == 1.0).all(axis=(0, 3))
    assert miss.any() and not miss.all()
    mu, S = _replay(L)
    expect = (S * (np.float32(spp) / np.float32(spp - 1))).astype(np.float32)
    r.variance = 1
    r.render(spp)
    var = r.variance()
    assert (var >= 0).all()
    assert _ulps(var, expect).max() <= 1
    assert (var[miss][:, :3] <= 2e-12).all(), float(var[miss][:, :3].max())
    assert (var[~miss][:, :3] > 0).any()


@pytest.mark.parametrize("order", (0, 1, 2))
def test_variance_of_a_tile_subset(order):
    """A TileShard share of a 64x48 frame (12 tiles): its pixels bit for bit the full frame's variance, the other pixels still the previous pass's"""
    from volren_amd.shard import TileShard
    full = scenes.hip_scene("c1", 64, 48)
    full.variance = 1
    full.render(8)
    want = full.variance()
    r = scenes.hip_scene("c1", 64, 48)
    r.variance = 1
    r.order_tiles = order
    r.seed = 99
    r.render(8)
    before = r.variance()
    assert not np.array_equal(before, want)
    mine = TileShard(64, 48, 3, 1).mine
    r.seed = full.seed
    r.reset()
    r.set_tiles(mine)
    r.render(8)
    got = r.variance()
    mask = np.zeros((48, 64), bool)
    for t in mine:
        ty, tx = divmod(t, 4)
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    assert 0 < mask.sum() < mask.size
    assert np.array_equal(_bits(got[mask]), _bits(want[mask]))
    assert np.array_equal(_bits(got[~mask]), _bits(before[~mask]))
    assert (got[mask] > 0).any()


def test_ragged_frame_partial_chunk_and_tile_subset_with_and_without_moments():
    """Every index rule of the accumulation pass at once (vr_tiles.h: pixel mapping, sample-pool slots): a frame ragged on both axes (40x24: 3 x 2
    tiles), 11 samples (the last chunk of a work unit partial at 8 and at 4 samples per unit), the tile list [0, 2, 5], variance off and on.  The two
    colour buffers bit for bit each other's and the oracle's, the moments bit for bit the host Welford replay's, unlisted tiles untouched."""
    w, h, spp, tiles = 40, 24, 11, [0, 2, 5]
    o = scenes.oracle_scene("c1", w, h)                      # smoke.brick
    L = _oracle_radiance(o, spp)
    mu, S = _replay(L)
    assert np.array_equal(_bits(mu), _bits(scenes.oracle_scene("c1", w, h).render(spp)))
    mask = np.zeros((h, w), bool)
    for t in tiles:
        ty, tx = divmod(t, 3)
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    assert 0 < mask.sum() < mask.size
    fbs = []
    for variance in (0, 1):
        r = scenes.hip_scene("c1", w, h)
        r.variance = variance
        r.set_tiles(tiles)
        r.render(spp)
        fb = r.framebuffer()
        print("variance", variance, "colour words off the oracle:", int((_bits(fb[mask]) != _bits(mu[mask])).sum()))
        assert np.array_equal(_bits(fb[mask]), _bits(mu[mask]))
        assert not fb[~mask].any()
        fbs.append(fb)
        if variance:
            var = r.variance()
            expect = (S * (np.float32(spp) / np.float32(spp - 1))).astype(np.float32)
            print("largest distance of the moments from the replay, ulps:", int(_ulps(var[mask], expect[mask]).max()))
            assert np.array_equal(_bits(var[mask]), _bits(expect[mask]))
            assert not var[~mask].any()
            assert (var[mask] > 0).any()
    assert np.array_equal(_bits(fbs[0]), _bits(fbs[1]))


def test_variance_in_the_tolerance_mode():
    """fast_math = 1 (no transfer function): variance on leaves the frame bit for bit, and the variance does not depend on the launch split"""
    r = scenes.hip_scene("c1", 256, 256)
    r.fast_math = 1
    r.render(24)
    fast = r.framebuffer()
    r.reset()
    r.variance = 1
    r.render(24)
    assert np.array_equal(_bits(r.framebuffer()), _bits(fast))
    ref = r.variance()
    assert (ref > 0).any()
    r.sample_pool_mb = 16
    r.reset()
    r.render(24)
    assert r.last_launches >= 2
    assert np.array_equal(_bits(r.variance()), _bits(ref)) and np.array_equal(_bits(r.framebuffer()), _bits(fast))
    r.sample_pool_mb = 65536
    r.reset()
    while r.sample < 24:
        r.trace()
    assert np.array_equal(_bits(r.variance()), _bits(ref)) and np.array_equal(_bits(r.framebuffer()), _bits(fast))
