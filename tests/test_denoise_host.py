"""CPU: the a-trous denoiser of the lane code (vr_denoise.h), host-compiled, against a float64 numpy statement of the filter (tests/hk_denoise.py),
on synthetic frames with hard edges and on frames of the oracle; its properties; and its noise reduction against a 1024-spp oracle frame."""
import numpy as np
import pytest

import hk_denoise
import hk_features
import scenes

SIGMA2 = (2.0, 3.0, 0.3, 0.5, 0.5)


def _close(host, spec, what):
    """host within 1e-5 of the spec, relative to the largest magnitude of each channel"""
    host = np.asarray(host, np.float64)
    spec = np.asarray(spec, np.float64)
    scale = np.abs(spec).reshape(-1, spec.shape[-1]).max(axis=0) if spec.ndim == 3 else np.abs(spec).max()
    err = (np.abs(host - spec) / np.maximum(scale, 1e-30)).max()
    assert err <= 1e-5, (what, err)


def synthetic(h=40, w=56, seed=5):
    """Noisy colour over hard edges in colour, coverage (environment | volume), depth, normal and albedo."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.where(x < w // 2, 0.2, 1.5)[..., None] * np.array([1.0, 0.8, 0.6])
    base = np.where((y > h // 3)[..., None], base, base[..., ::-1] * 2.0)
    color = np.concatenate([base * (1 + 0.3 * rng.standard_normal((h, w, 3))), np.ones((h, w, 1))], axis=-1)
    var = np.concatenate([(0.3 * base) ** 2 * (1 + 0.2 * rng.random((h, w, 3))), np.zeros((h, w, 1))], axis=-1)
    feat = np.zeros((h, w, 8))
    vol = (x - w // 2) ** 2 + (y - h // 2) ** 2 < (0.4 * h) ** 2
    feat[..., 0:3] = np.where((x < w // 3)[..., None], [0.9, 0.9, 0.9], [0.3, 0.6, 0.9])
    feat[..., 3] = np.where(vol, 0.25 + 0.75 * rng.random((h, w)), 0.0)
    n = np.stack([np.where(y < h // 2, 1.0, 0.0), np.where(y < h // 2, 0.0, 0.8), 0.3 * rng.standard_normal((h, w))], -1)
    feat[..., 4:7] = n
    feat[..., 7] = np.where(x + y < (w + h) // 2, 2.0, 5.0) + 0.05 * rng.random((h, w))
    feat[~vol] = 0.0
    feat[h // 2, w // 2, 4:7] = 0.0                     # a covered pixel whose normal averaged to 0 (w_n = 1 against it)
    return color.astype(np.float32), var.astype(np.float32), feat.astype(np.float32)


_ORACLE = {}


def oracle_inputs(name, w, h, spp):
    """(mean, unbiased variance, features, n) of an oracle frame: the per-sample radiances replayed through the accumulation pass's arithmetic
    (test_gpu_features._replay), the features from the host-built feature pass."""
    key = (name, w, h, spp)
    if key not in _ORACLE:
        from test_gpu_features import _oracle_radiance, _replay
        o = scenes.oracle_scene(name, w, h)
        L = _oracle_radiance(o, spp)
        mu, S = _replay(L)
        var = (S * (np.float32(spp) / np.float32(spp - 1))).astype(np.float32)
        _ORACLE[key] = (mu, var, hk_features.feature_pass(o, spp), spp)
    return _ORACLE[key]


def _inputs(kind):
    if kind == "synthetic":
        c, v, f = synthetic()
        return c, v, f, 8
    return oracle_inputs(kind, 48, 32, 8)


@pytest.mark.parametrize("kind", ("synthetic", "c1", "c3"))
@pytest.mark.parametrize("sigma", (hk_denoise.DEFAULT_SIGMA, SIGMA2))
def test_host_build_matches_the_float64_spec(kind, sigma):
    c, v, f, n = _inputs(kind)
    vh, gh = hk_denoise.prepare(v, f, n)
    vs, gs = hk_denoise.spec_prepare(v, f, n)
    _close(vh, vs, "prepare v")
    assert np.abs(gh - gs).max() <= 1e-6
    # each iteration from the same float32 inputs (the host's previous iteration)
    cc, vv = c, vh
    for k in range(5):
        ch, vh2 = hk_denoise.atrous(cc, vv, gh, 1 << k, sigma)
        cs, vs2 = hk_denoise.spec_atrous(cc, vv, gh, 1 << k, sigma)
        _close(ch, cs, (kind, k, "colour"))
        _close(vh2, vs2, (kind, k, "variance"))
        cc, vv = ch, vh2
    # and the whole filter, iterations chained in float64
    _close(hk_denoise.denoise(c, v, f, n, 5, sigma), hk_denoise.spec_denoise(c, v, f, n, 5, sigma), (kind, "N=5"))
    assert np.array_equal(hk_denoise.denoise(c, v, f, n, 5, sigma), cc)


@pytest.mark.parametrize("kind", ("synthetic", "c1"))
def test_zero_iterations_are_the_identity(kind):
    c, v, f, n = _inputs(kind)
    assert np.array_equal(hk_denoise.denoise(c, v, f, n, 0).view(np.uint32), c.view(np.uint32))


def test_a_constant_image_stays_constant():
    _, v, f = synthetic()
    c = np.full(v.shape, 0.37, np.float32)
    c[..., 3] = 1.0
    out = hk_denoise.denoise(c, v, f, 8, 10)
    assert np.abs(out[..., :3] - 0.37).max() <= 1e-6 * 0.37 * 10 and np.abs(out[..., 3] - 1.0).max() <= 1e-6


def test_a_colour_step_without_variance_does_not_blur():
    h, w = 24, 32
    c = np.zeros((h, w, 4), np.float32)
    c[:, w // 2:, :3] = 1.0
    c[..., 3] = 1.0
    var = np.zeros((h, w, 4), np.float32)
    f = np.zeros((h, w, 8), np.float32)                # no volume: only colour and coverage guide
    out = hk_denoise.denoise(c, var, f, 8, 5)
    assert np.array_equal(out, c)


def test_a_coverage_edge_bleeds_little():
    """Left half environment (coverage 0, bright, equal luminance noise), right half volume (coverage 1, dark): the colour weight alone lets
    everything through (huge variance); the coverage weight must keep the halves apart -- w_k = exp(-1 / 0.25) = 0.018 per tap."""
    rng = np.random.default_rng(2)
    h, w = 24, 32
    c = np.zeros((h, w, 4), np.float32)
    c[:, : w // 2, :3] = 2.0
    c[:, w // 2:, :3] = 0.5
    c[..., :3] *= (1 + 0.05 * rng.standard_normal((h, w, 1))).astype(np.float32)
    c[..., 3] = 1.0
    var = np.full((h, w, 4), 100.0, np.float32)
    var[..., 3] = 0
    f = np.zeros((h, w, 8), np.float32)
    f[:, w // 2:, 3] = 1.0
    f[:, w // 2:, 0:3] = 0.8
    f[:, w // 2:, 4:7] = (0, 0, 1)
    f[:, w // 2:, 7] = 3.0
    out = hk_denoise.denoise(c, var, f, 8, 5)
    env, vol = out[:, : w // 2, :3].mean(axis=-1), out[:, w // 2:, :3].mean(axis=-1)
    # next to the edge, the other side's share of the result stays below 10 %: |out - own level| <= 0.1 * 1.5
    assert np.abs(env - 2.0).max() <= 0.15 and np.abs(vol - 0.5).max() <= 0.15, (np.abs(env - 2.0).max(), np.abs(vol - 0.5).max())
    plain = hk_denoise.denoise(c, var, np.zeros_like(f), 8, 5)         # the same frame without the coverage edge: it blurs
    assert np.abs(plain[:, w // 2:, :3].mean(axis=-1) - 0.5).max() > 0.3


@pytest.mark.parametrize("iterations", (1, 3, 5))
def test_output_depends_on_the_footprint_only(iterations):
    """Pixel p's result after N iterations depends on pixels within 2 (1 + 2 + ... + 2^(N-1)) + N of p (taps + the 3x3 variance prefilter):
    a change farther away leaves it bit for bit, a change inside changes it."""
    c, v, f = synthetic(64, 96)
    base = hk_denoise.denoise(c, v, f, 8, iterations)
    reach = 2 * (2 ** iterations - 1) + iterations
    py, px = 30, 10
    qx = px + reach + 1
    assert qx < 96
    for arr in (c, v, f):
        a = arr.copy()
        a[py, qx] = a[py, qx] * 3 + 1
        args = [a if arr is x else x for x in (c, v, f)]
        out = hk_denoise.denoise(*args, 8, iterations)
        assert np.array_equal(out[py, : px + 1], base[py, : px + 1])
        assert not np.array_equal(out[py, qx], base[py, qx])
    a = c.copy()
    a[py, px + 2 ** (iterations - 1) * 2] += 5.0           # the last iteration's outermost tap
    assert not np.array_equal(hk_denoise.denoise(a, v, f, 8, iterations)[py, px], base[py, px])


def test_noise_reduction_on_an_oracle_frame():
    """8 spp of c1 at 64x48 with variance and features, against 1024 spp of another seed: measured ratio 0.515 (defaults); bound 0.65."""
    mu, var, feat, n = oracle_inputs("c1", 64, 48, 8)
    o = scenes.oracle_scene("c1", 64, 48)
    o.seed = 1234567
    o.render(1024)
    ref = o.fb[..., :3].copy()
    raw = scenes.rel_l2(mu[..., :3], ref)
    den = scenes.rel_l2(hk_denoise.denoise(mu, var, feat, n)[..., :3], ref)
    assert den <= 0.65 * raw, (raw, den)


# ---- hostile inputs and the limits of denoise_sigma ----------------------------------------------------------------------------------------------
def _f32_dot(a, b):
    """vr_math.h dot in float32: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)) (a float64 product of two floats is exact)"""
    f = np.float32
    xy = (a[..., 0].astype(f) * b[..., 0].astype(f)).astype(np.float64)
    s = (a[..., 1].astype(np.float64) * b[..., 1] + xy).astype(f)
    return (a[..., 2].astype(np.float64) * b[..., 2] + s.astype(np.float64)).astype(f)


def unit_normal_over_one(seed=0):
    """A feature normal whose guide (normalised in float32) has a float32 dot with itself of more than 1"""
    rng = np.random.default_rng(seed)
    for _ in range(1000):
        n = rng.standard_normal((64, 3)).astype(np.float32)
        f = np.zeros((1, 64, 8), np.float32)
        f[0, :, 4:7] = n
        g = hk_denoise.prepare(np.zeros((1, 64, 4), np.float32), f, 1)[1][0, :, 4:7]
        d = _f32_dot(g, g)
        if (d > 1).any():
            return n[int(np.argmax(d))]
    raise AssertionError("no normal found")


def hostile(h=33, w=47, seed=11, equal_normals=None):
    """Colour from 1e-6 to 1e5 (blocks of one level, each with its noise), variance from 0 to 1e10, fractional coverage, depth 0 on some covered
    pixels, normals that are all zero, exactly equal (a guide whose float32 dot with itself exceeds 1), nearly equal, and random."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    level = 10.0 ** rng.uniform(-6, 5, (h // 8 + 1, w // 8 + 1, 3))[y // 8, x // 8]
    color = np.concatenate([level * (1 + 0.2 * rng.standard_normal((h, w, 3))).clip(0.01), rng.integers(0, 9, (h, w, 1)) / 8.0], axis=-1)
    var = np.concatenate([(10.0 ** rng.uniform(-8, 10, (h, w, 3))) * (rng.random((h, w, 3)) > 0.1), np.zeros((h, w, 1))], axis=-1)
    feat = np.zeros((h, w, 8))
    feat[..., 0:3] = np.where((x < w // 2)[..., None], [0.5, 0.5, 0.5], rng.random((h, w, 3)))
    feat[..., 3] = rng.integers(0, 9, (h, w)) / 8.0                            # 0, 1/8, ..., 1: fractional coverage, some pixels uncovered
    n0 = unit_normal_over_one() if equal_normals is None else np.asarray(equal_normals, np.float32)
    band = (y * 4) // h                                                         # 0 zero normals, 1 exactly equal, 2 nearly equal, 3 random
    feat[..., 4:7] = np.where((band == 1)[..., None], n0, 0.0)
    near = n0 * (1 + 1e-6 * rng.standard_normal((h, w, 3)))
    feat[..., 4:7] = np.where((band == 2)[..., None], near, feat[..., 4:7])
    feat[..., 4:7] = np.where((band == 3)[..., None], rng.standard_normal((h, w, 3)), feat[..., 4:7])
    feat[..., 7] = np.where(rng.random((h, w)) < 0.2, 0.0, rng.uniform(0.5, 4.0, (h, w)))     # depth 0 on a fifth of the pixels
    feat[feat[..., 3] == 0] = 0.0
    return color.astype(np.float32), var.astype(np.float32), feat.astype(np.float32)


def _spec_per_iteration(c, v, f, n, sigma, iterations=5):
    vh, gh = hk_denoise.prepare(v, f, n)
    vs, _ = hk_denoise.spec_prepare(v, f, n)
    _close(vh, vs, "prepare v")
    cc, vv = c, vh
    for k in range(iterations):
        ch, vh2 = hk_denoise.atrous(cc, vv, gh, 1 << k, sigma)
        assert np.isfinite(ch).all() and np.isfinite(vh2).all(), (sigma, k)
        cs, vs2 = hk_denoise.spec_atrous(cc, vv, gh, 1 << k, sigma)
        _close(ch, cs, (sigma, k, "colour"))
        _close(vh2, vs2, (sigma, k, "variance"))
        cc, vv = ch, vh2
    out = hk_denoise.denoise(c, v, f, n, iterations, sigma)
    assert np.array_equal(out, cc) and np.isfinite(out).all()
    return out


@pytest.mark.parametrize("n", (1, 8))
@pytest.mark.parametrize("sigma", (hk_denoise.DEFAULT_SIGMA, SIGMA2))
def test_host_build_matches_the_float64_spec_on_hostile_inputs(n, sigma):
    c, v, f = hostile()
    g = hk_denoise.prepare(v, f, n)[1]
    band = (np.arange(c.shape[0]) * 4) // c.shape[0]
    eq = g[band == 1][f[band == 1][..., 3] > 0][:, 4:7]
    assert len(eq) > 50 and (_f32_dot(eq, eq) > 1).all()                  # the exactly-equal band: w_n's dot exceeds 1 on every pair
    assert (f[..., 3] > 0).any() and ((f[..., 3] > 0) & (f[..., 3] < 1)).any() and ((f[..., 3] > 0) & (f[..., 7] == 0)).any()
    assert c[..., :3].min() < 1e-5 and c[..., :3].max() > 1e4 and v.max() > 1e9
    out = _spec_per_iteration(c, v, f, n, sigma)
    assert not np.array_equal(out, c)


def test_the_normal_weight_never_exceeds_one():
    """Two covered pixels, equal in everything but the alpha channel (0 and 1), whose guide normals are equal and have a float32 dot of more than
    1.  Pixel 0's alpha after one iteration is w / (w_centre + w) with w_centre = (3/8)^2 and w = (1/4)(3/8) w_n: 0.4 exactly when w_n = 1.
    Before the clamp, w_n = (1 + 2^-22)^sigma_n > 1, and inf from sigma_n of about 3.7e8 on (the alpha NaN)."""
    nrm = unit_normal_over_one()
    c = np.full((1, 2, 4), 0.5, np.float32)
    c[0, 0, 3], c[0, 1, 3] = 0.0, 1.0
    f = np.zeros((1, 2, 8), np.float32)
    f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7] = 0.5, 1.0, nrm, 2.0
    g = hk_denoise.prepare(np.zeros((1, 2, 4), np.float32), f, 4)[1]
    assert _f32_dot(g[0, 0, 4:7], g[0, 1, 4:7]) > 1
    want = np.float32(0.09375) / np.float32(0.234375)
    lo, hi = hk_denoise.sigma_range()
    for sn in (lo, 0.5, 1.0, 16.0, 1e6, 5e8, 1e9, hi):
        sg = (4.0, sn, 0.1, 0.25, 0.2)
        out = hk_denoise.denoise(c, np.zeros((1, 2, 4), np.float32), f, 4, 1, sg)
        assert out[0, 0, 3] == want and out[0, 1, 3] == np.float32(1) - want, (sn, out[0, :, 3])
        assert np.isfinite(out).all()


def test_sigma_range():
    lo, hi = hk_denoise.sigma_range()
    assert lo == 2.0 ** -60 and hi == 2.0 ** 60
    assert np.float32(lo) * np.float32(lo) >= np.finfo(np.float32).tiny        # sigma_a^2 stays a normal float
    text = open(scenes.ROOT + "/include/volren_amd.h").read() + open(scenes.ROOT + "/README.md").read()
    assert text.count("[2^-60, 2^60]") >= 2


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("end", ("smallest", "largest"))
def test_sigma_limits_give_finite_output(which, end):
    """Each sigma alone at the smallest and the largest value vr_set_float accepts, the others at their defaults: every output finite, on
    synthetic() and on the hostile frame (n = 1 and 8), and the host build matches the float64 spec per iteration -- except at sigma_n = 2^60,
    where any rounding of dot(g_p, g_q) below 1 turns w_n from 1 into 0 (float32 and float64 round differently): there the output is checked
    to be finite and a convex combination of the frame's colours."""
    lo, hi = hk_denoise.sigma_range()
    sg = list(hk_denoise.DEFAULT_SIGMA)
    sg[which] = lo if end == "smallest" else hi
    sg = tuple(sg)
    ill = which == 1 and end == "largest"
    frames = [(*synthetic(), 8), (*hostile(), 1), (*hostile(seed=3), 8)]
    for c, v, f, n in frames:
        if ill:
            out = hk_denoise.denoise(c, v, f, n, 5, sg)
            assert np.isfinite(out).all(), sg
            tol = 1e-6 * np.abs(c).reshape(-1, 4).max(axis=0)
            assert ((out >= c.reshape(-1, 4).min(axis=0) - tol) & (out <= c.reshape(-1, 4).max(axis=0) + tol)).all()   # convex combinations
        else:
            _spec_per_iteration(c, v, f, n, sg)
