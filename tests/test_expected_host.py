"""CPU: the expected-value feature pass (volren_amd/csrc/vr_expected.h expected_pixel), host-compiled (tests/hostkernel/expected_host.cpp), against
a float64 numpy statement of its definition (tests/hk_expected.py spec_expected); as the limit of the stochastic feature pass; as a guide of the
a-trous filter and of the temporal accumulation in place of the stochastic one; and on cameras and settings at the edge of its domain."""
import numpy as np
import pytest

import hk_denoise
import hk_expected as he
import hk_features
import hk_temporal as ht
import scenes
from hk_common import same as _same
from test_denoise_host import oracle_inputs

W, H = 64, 48
CH = ("albedo.r", "albedo.g", "albedo.b", "coverage", "normal.x", "normal.y", "normal.z", "depth")

# ---- 1: the host build against the float64 statement -------------------------------------------------------------------------------------------------
# Largest absolute difference per channel over the compared pixels, measured with this very test (see its docstring): ALL = every compared pixel,
# SOLID = those with coverage >= 0.01.
MEASURED_ALL = {
    ("c1", 1): (6.56e-07, 6.56e-07, 6.56e-07, 8.95e-06, 6.04e-02, 1.20e-02, 5.74e-02, 5.08e-04),
    ("c1", 2): (9.00e-01, 9.00e-01, 9.00e-01, 3.32e-06, 1.88e-02, 1.00e+00, 3.68e-02, 1.50e+00),
    ("c3", 1): (1.35e-05, 2.93e-06, 8.49e-06, 8.57e-06, 1.07e-01, 1.20e-02, 1.01e-01, 8.97e-04),
    ("c3", 2): (3.39e-06, 3.17e-06, 5.28e-06, 3.24e-06, 1.88e-02, 1.00e+00, 3.68e-02, 1.50e+00),
    ("c4_64", 1): (8.00e-01, 8.00e-01, 8.00e-01, 2.89e-06, 8.15e-01, 5.78e-01, 4.02e-02, 1.21e+00),
    ("c4_64", 2): (4.77e-07, 4.77e-07, 4.77e-07, 1.47e-06, 3.95e-04, 8.91e-04, 7.71e-04, 1.38e-05),
    ("c5_64", 1): (3.58e-07, 3.58e-07, 3.58e-07, 2.37e-06, 1.25e-04, 1.70e-05, 9.38e-05, 2.45e-06),
    ("c5_64", 2): (4.77e-07, 4.77e-07, 4.77e-07, 1.42e-06, 2.34e-04, 2.46e-04, 1.60e-04, 1.17e-05),
}
MEASURED_SOLID = {
    ("c1", 1): (6.56e-07, 6.56e-07, 6.56e-07, 8.95e-06, 3.74e-05, 6.63e-05, 2.09e-05, 9.59e-07),
    ("c1", 2): (1.07e-06, 1.07e-06, 1.07e-06, 3.32e-06, 1.51e-04, 3.08e-05, 2.20e-05, 2.03e-06),
    ("c3", 1): (1.35e-05, 2.93e-06, 8.49e-06, 8.57e-06, 3.57e-05, 6.01e-05, 1.62e-05, 1.30e-06),
    ("c3", 2): (3.39e-06, 3.17e-06, 5.28e-06, 3.24e-06, 1.22e-04, 2.50e-05, 2.20e-05, 1.64e-06),
    ("c4_64", 1): (2.98e-07, 2.98e-07, 2.98e-07, 2.89e-06, 3.51e-06, 4.05e-06, 2.29e-06, 5.11e-07),
    ("c4_64", 2): (4.77e-07, 4.77e-07, 4.77e-07, 1.47e-06, 1.64e-06, 1.70e-06, 1.55e-06, 9.03e-07),
    ("c5_64", 1): (3.58e-07, 3.58e-07, 3.58e-07, 2.37e-06, 3.80e-06, 5.72e-06, 5.99e-06, 1.05e-06),
    ("c5_64", 2): (4.77e-07, 4.77e-07, 4.77e-07, 1.42e-06, 1.89e-06, 1.78e-06, 2.01e-06, 6.90e-07),
}


@pytest.mark.parametrize("rays", (1, 2))
@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
def test_host_build_matches_the_float64_statement(name, rays):
    """smoke.brick, + lut.txt, a dense fp16 grid, brick grids with an emission grid; 64x48.  Compared: every pixel in which both builds ran the same
    number of steps on every sub-ray -- a different count means one of them met the T <= 2^-10 cut a step before the other -- which must be all but
    1 % of the covered pixels (measured: 1 pixel of c5_64 at 2 x 2 rays, none elsewhere; the step counts m agree everywhere).
    Asserted at four times the measured largest absolute difference per channel (MEASURED_ALL above; float32 sums of up to 185 terms per sub-ray).
    What the ALL figures of the ratio channels show -- albedo, normal and depth up to 0.9, 1.0 and 1.5 -- are pixels at the silhouette with a coverage
    of 1e-6 and less: 1 - e carries an absolute error of 2^-25 per step, so where sigma h is of that size the weights are known to no digit (and a
    pixel may be covered in one build and empty in the other), and a ratio of two such sums says nothing.  The filter weighs these pixels by their
    coverage.  So the same is asserted once more on the pixels with a coverage of 0.01 and more (MEASURED_SOLID): there the worst channel, a normal
    component, is within 1.6e-4, coverage within 9e-6, depth within 2.1e-6 (volume widths) and albedo within 1.4e-5."""
    o = scenes.oracle_scene(name, W, H)
    got, m, steps, _ = he.expected_pass(o, rays, with_info=True)
    ref, m64, steps64 = he.spec_expected(o, rays)
    assert _same(got, he.expected_pass(o, rays))                                    # the plain entry point returns the same frame
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
    print("all  :", " ".join("%.2e" % x for x in d_all))
    print("solid:", " ".join("%.2e" % x for x in d_solid))
    for c in range(8):
        assert d_all[c] <= 4.0 * MEASURED_ALL[(name, rays)][c], (CH[c], d_all[c])
        assert d_solid[c] <= 4.0 * MEASURED_SOLID[(name, rays)][c], (CH[c], d_solid[c])


def test_analytic_gradient_is_the_derivative_of_the_trilinear_filter():
    """the float64 statement's own gradient against a central difference of hk_features.trilinear inside one cell (the interpolant is a polynomial
    there: the difference quotient of a trilinear function along an axis is exact)"""
    rng = np.random.default_rng(5)
    grid = hk_features.decoded_grid(scenes.oracle_scene("c1", 8, 8).density)
    nz, ny, nx = grid.shape
    p = np.floor(rng.uniform(2, min(nx, ny, nz) - 3, (2000, 3))) + 0.5 + rng.uniform(0.2, 0.8, (2000, 3))
    v, f = he.corners(grid, p)
    val, g = he.value_and_gradient(v, f)
    assert np.allclose(val, hk_features.trilinear(grid, p), rtol=1e-12, atol=1e-12)
    for a in range(3):
        e = np.zeros(3)
        e[a] = 0.1
        assert np.allclose(g[:, a], (hk_features.trilinear(grid, p + e) - hk_features.trilinear(grid, p - e)) / 0.2, rtol=1e-9, atol=1e-9)
    assert (np.abs(g).sum(axis=1) > 0).mean() > 0.1


# ---- 2: the limit of the stochastic pass ----------------------------------------------------------------------------------------------------------------
def _against_stochastic(e, s):
    both = (e[..., 3] > 0.2) & (s[..., 3] > 0.2)
    return (float(np.abs(e[..., 3] - s[..., 3]).mean()), float((np.abs(e[..., 7] - s[..., 7])[both] / s[..., 7][both]).mean()),
            float(np.abs(e[..., 4:7] - s[..., 4:7])[both].mean()))


@pytest.mark.parametrize("name", ("c2", "c3"))
def test_it_is_the_limit_of_the_stochastic_pass(name):
    """Against hk_features.feature_pass(o, 512) at 64x48: mean |coverage difference| over all pixels; mean relative depth difference and mean
    |normal difference| over the pixels where both coverages exceed 0.2.  4 x 4 rays are closer than 1 in all three, and 2 x 2 rays stay within
    twice the float64 prototype's figures for c2 (0.0022, 0.17 %, 0.053): 0.0044, 0.34 %, 0.106.  The host build gives
                 coverage   depth      normal
      c2  1 ray  0.00590    0.00417    0.1245
      c2  2 x 2  0.00224    0.00171    0.0578
      c2  4 x 4  0.00187    0.00146    0.0424
      c3  1 ray  0.00581    0.00398    0.1223
      c3  2 x 2  0.00225    0.00182    0.0571
      c3  4 x 4  0.00194    0.00163    0.0423"""
    o = scenes.oracle_scene(name, W, H)
    s = hk_features.feature_pass(o, 512)
    d = {rays: _against_stochastic(he.expected_pass(o, rays), s) for rays in (1, 2, 4)}
    for rays in (1, 2, 4):
        print("%s rays %d: coverage %.5f depth %.5f normal %.4f" % ((name, rays) + d[rays]))
    assert all(d[4][k] < d[1][k] for k in range(3))
    assert d[2][0] <= 0.0044 and d[2][1] <= 0.0034 and d[2][2] <= 0.106


# ---- 3: a better guide than the one it replaces ----------------------------------------------------------------------------------------------------------
_REFERENCE = {}


def _reference(name):
    if name not in _REFERENCE:
        o = scenes.oracle_scene(name, W, H)
        o.seed = 1234567
        _REFERENCE[name] = o.render(1024).copy()
    return _REFERENCE[name]


@pytest.mark.parametrize("spp", (2, 16))
@pytest.mark.parametrize("name", ("c2", "c3"))
def test_it_guides_the_filter_better_than_the_frames_own_features(name, spp):
    """Oracle frames at 64x48 (seed 42) through the host build of the filter at default sigmas, relative L2 of RGB against 1024 spp of seed 1234567:
    the guide of 2 x 2 expected rays against the frame's own stochastic features (spp samples).  No margin.  Measured (own guide -> expected guide):
      c2  2 spp  0.1200 -> 0.1012      c2 16 spp  0.0552 -> 0.0495
      c3  2 spp  1.3510 -> 0.6179      c3 16 spp  0.3217 -> 0.2887"""
    color, var, feat, n = oracle_inputs(name, W, H, spp)
    ref = _reference(name)[..., :3]
    guide = he.expected_pass(scenes.oracle_scene(name, W, H), 2)
    own = scenes.rel_l2(hk_denoise.denoise(color, var, feat, n)[..., :3], ref)
    exp = scenes.rel_l2(hk_denoise.denoise(color, var, guide, n)[..., :3], ref)
    print("%s %d spp: own guide %.4f, expected guide %.4f" % (name, spp, own, exp))
    assert exp <= own


# ---- 4: edge cases ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_camera_looking_away_sees_nothing():
    o = scenes.oracle_scene("c1", 32, 24)
    o.cam_dir = tuple(-x for x in o.cam_dir)
    assert not he.expected_pass(o, 2).any()


def test_a_camera_inside_the_volume():
    o = scenes.oracle_scene("c1", 32, 24)
    o.cam_pos, o.cam_dir, o.cam_fov = (0.05, 0.0, -0.1), (0.4, 0.2, 1.0), 80.0
    out = he.expected_pass(o, 2)
    assert np.isfinite(out).all() and (out[..., 3] > 0).any()
    assert out[out[..., 3] > 0][:, 7].min() < 0.1                       # collisions right in front of the camera


def test_a_camera_36000_volume_widths_away_returns():
    o = scenes.oracle_scene("c1", 16, 12)
    near = o.cam_pos
    o.cam_pos, o.cam_fov = tuple(36000.0 * x for x in near), 40.0 / 36000.0
    out, m, steps, _ = he.expected_pass(o, 2, with_info=True)
    assert np.isfinite(out).all() and m.max() <= he.MAX_STEPS and (steps <= m).all()
    print("far camera: %d covered pixels, longest sub-ray %d steps" % (int((out[..., 3] > 0).sum()), int(m.max())))


def test_the_clip_box_removes_coverage_outside_it():
    o = scenes.oracle_scene("c1", W, H)
    full = he.expected_pass(o, 1)
    o.vol_clip_min, o.vol_clip_max = (0.0, 0.0, 0.0), (1.0, 0.45, 1.0)             # the upper part of the smoke column cut away
    cropped = he.expected_pass(o, 1)
    ref, _, _ = he.spec_expected(o, 1)
    assert np.abs(cropped[..., 3] - ref[..., 3]).max() <= 4 * 8.95e-6               # the crop acts as the float64 statement says (c1's coverage bound)
    # (a cropped segment is cut into steps of its own, so where both see the same smoke the two quadratures differ a little: 0.0014 at most here)
    assert (cropped[..., 3] <= full[..., 3] + 0.01).all()
    gone = (full[..., 3] > 0.01) & (cropped[..., 3] == 0)
    assert gone.sum() > 20 and (cropped[..., 3] > 0.01).sum() > 20
    # ... and they are the rows above the crop: no covered pixel of the cropped frame lies above the highest row that lost none
    rows = np.flatnonzero((cropped[..., 3] > 0).any(axis=1))
    assert rows.max() < np.flatnonzero(gone.any(axis=1)).max()


def test_a_density_scale_of_zero_gives_zeros():
    for name in ("c1", "c4_64"):
        o = scenes.oracle_scene(name, 32, 24)
        o.density_scale = 0.0
        assert not he.expected_pass(o, 2).any()


@pytest.mark.parametrize("name", ("c1", "c3"))
def test_two_calls_give_the_same_bits_and_no_seed_matters(name):
    o = scenes.oracle_scene(name, 32, 24)
    a = he.expected_pass(o, 3)
    o.seed = 7
    o.integrator = 1
    assert _same(a, he.expected_pass(o, 3)) and (a[..., 3] > 0).any()


# ---- 5: no restarts from guide noise ------------------------------------------------------------------------------------------------------------------------
def test_a_fixed_camera_never_restarts_a_pixel():
    """8 frames of 2 spp of c2 at 64x48 (seeds 100 .. 107, test_moments_host's frames), fixed camera, alpha 0.1, the guide rendered afresh for every
    frame.  With the expected guide every pixel's history is i + 1 frames long after frame i.  With the stochastic features of 2 spp the depth and
    coverage test restarts pixels in every frame: after frame 7, 9.0 % of the pixels have a history shorter than 8 (measured)."""
    from test_moments_host import _oracle_frames
    frame_of, cam = _oracle_frames(2, 8)
    guide = he.expected_pass(scenes.oracle_scene("c2", W, H), 2)
    steady, noisy = ht.Replay(), ht.Replay()
    for i in range(8):
        color, var, feat = frame_of(i)
        assert _same(guide, he.expected_pass(scenes.oracle_scene("c2", W, H), 2))        # afresh, and the same
        n_steady = steady.frame(cam, color, var, guide, 2, 0.1, iterations=0)[2]
        n_noisy = noisy.frame(cam, color, var, feat, 2, 0.1, iterations=0)[2]
        assert (n_steady == i + 1).all(), (i, int((n_steady != i + 1).sum()))
    short = float((n_noisy < 8).mean())
    print("stochastic guide: %.1f %% of the pixels with a history shorter than 8 after frame 7" % (100.0 * short))
    assert short > 0


# ---- 6: the 1-spp sequence, recorded only -------------------------------------------------------------------------------------------------------------------
def test_one_sample_per_pixel_with_the_expected_guide_is_recorded():
    """test_moments_host's sequence (16 frames x 1 spp, c2 at 64x48, seeds 100 .. 115, moments on, relative L2 against 1024 spp of seed 777) with
    the guide of 2 x 2 expected rays in place of features of 1 spp.  Nothing is asserted but that the run is finite.  Measured, with moments:
      features of 1 spp   frame 0 0.1565   mean of frames 10 .. 15 0.1471
      expected guide      frame 0 0.1278   mean of frames 10 .. 15 0.0538"""
    import test_moments_host as tm
    o = scenes.oracle_scene("c2", W, H)
    o.seed = 777
    reference = o.render(1024).copy()
    frame_of, cam = tm._oracle_frames(1, tm.FRAMES)
    guide = he.expected_pass(scenes.oracle_scene("c2", W, H), 2)
    err = {}
    for what in ("features of 1 spp", "expected guide"):
        rp = tm.hm.Replay()
        e = []
        for i in range(tm.FRAMES):
            color, var, feat = frame_of(i)
            out = rp.frame(cam, color, var, feat if what[0] == "f" else guide, 1, 0.1)[4]
            e.append(scenes.rel_l2(out[..., :3], reference[..., :3]))
        err[what] = np.asarray(e)
        print("%-18s frame 0 %.4f   mean of frames 10 .. 15 %.4f   (%s)" % (what, e[0], float(np.mean(e[10:])), " ".join("%.4f" % x for x in e)))
    assert all(np.isfinite(e).all() for e in err.values())
