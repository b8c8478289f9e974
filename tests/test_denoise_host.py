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
