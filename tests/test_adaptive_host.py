"""CPU: the adaptive-sampling lane code (vr_adaptive.h) built for the host, against a float64 statement of the error estimate, on ordinary and hostile
frames, and its schedule functions."""
import numpy as np
import pytest

import hk_adaptive as ha


def _frame(h, w, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    mu = (rng.random((h, w, 4)) * scale).astype(np.float32)
    S = (rng.random((h, w, 4)) * scale * scale * 0.3).astype(np.float32)
    return mu, S


def _close(got, want, rtol=1e-6):
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=0)


@pytest.mark.parametrize("w,h", ((16, 16), (72, 56), (1, 1), (17, 33), (50, 37)))
@pytest.mark.parametrize("n", (2, 3, 8, 64, 1024))
def test_tile_error_matches_the_float64_statement(w, h, n):
    mu, S = _frame(h, w, w * 1000 + h + n)
    _close(ha.tile_error(mu, S, n), ha.spec_tile_error(mu, S, n))
    _close(ha.pixel_error(mu, S, n), ha.spec_pixel_error(mu, S, n))


def test_ragged_counts_and_hdr_values():
    w, h = 72, 56
    mu, S = _frame(h, w, 5, scale=1e4)
    counts = np.arange(20, dtype=np.int32).reshape(4, 5) * 7 + 2
    _close(ha.tile_error(mu, S, counts), ha.spec_tile_error(mu, S, counts))
    mu2, S2 = _frame(h, w, 6, scale=1e-5)
    _close(ha.tile_error(mu2, S2, counts), ha.spec_tile_error(mu2, S2, counts))


def test_one_sample_is_infinite_and_zero_counts_too():
    mu, S = _frame(32, 32, 1)
    for n in (0, 1):
        assert np.isposinf(ha.tile_error(mu, S, n)).all()
    counts = np.array([[1, 2], [0, 9]], np.int32)
    e = ha.tile_error(mu, S, counts)
    assert np.isposinf(e[0, 0]) and np.isposinf(e[1, 0]) and np.isfinite(e[0, 1]) and np.isfinite(e[1, 1])


def test_zero_mean_zero_variance_and_negative_moments():
    mu, S = _frame(16, 16, 2)
    zero = np.zeros_like(mu)
    e = ha.pixel_error(zero, S, 8)                          # black pixels: relative to the floor 2^-10
    _close(e, ha.spec_pixel_error(zero, S, 8))
    assert (e > 0).all() and np.float32(ha.lib().hk_adaptive_floor()) == np.float32(2.0 ** -10)
    assert (ha.pixel_error(mu, np.zeros_like(S), 8) == 0).all()          # no variance: converged at any threshold > 0
    neg = np.full_like(S, -1e-9)                            # rounding can leave S slightly negative: taken as 0
    assert (ha.pixel_error(mu, neg, 8) == 0).all()
    mixed = S.copy()
    mixed[..., 1] = -1e-9
    _close(ha.pixel_error(mu, mixed, 8), ha.spec_pixel_error(mu, mixed, 8))
    assert (ha.tile_error(zero, np.zeros_like(S), 8) == 0).all()


def test_nan_propagates_to_the_tile():
    mu, S = _frame(32, 48, 3)
    S[5, 20, 0] = np.nan                                    # tile (0, 1)
    mu[30, 40, 2] = np.nan                                  # tile (1, 2)
    e = ha.tile_error(mu, S, 16)
    assert np.isnan(e[0, 1]) and np.isnan(e[1, 2])
    assert np.isfinite(e[0, 0]) and np.isfinite(e[1, 1])
    assert np.isnan(ha.spec_tile_error(mu, S, 16)[0, 1])
    assert not ha.converged(float(e[0, 1]), 1e30)


def test_partial_edge_tiles_see_only_their_pixels():
    w, h = 40, 20                                           # tiles: 3 x 2, the last column 8 wide, the top row 4 high
    mu, S = _frame(h, w, 4)
    base = ha.tile_error(mu, S, 8)
    big = np.zeros((32, 48, 4), np.float32)
    bigS = np.full((32, 48, 4), 1e6, np.float32)            # huge error outside the frame must not leak in
    big[:h, :w], bigS[:h, :w] = mu, S
    assert np.array_equal(ha.tile_error(big, bigS, 8)[:, :], ha.tile_error(big, bigS, 8))
    assert np.array_equal(base, ha.tile_error(np.ascontiguousarray(big[:h, :w]), np.ascontiguousarray(bigS[:h, :w]), 8))
    e_px = ha.pixel_error(mu, S, 8)
    assert base[1, 2] == e_px[16:20, 32:40].max() and base[0, 2] == e_px[0:16, 32:40].max()


def test_error_from_variance_equals_error_from_moments():
    mu, S = _frame(37, 50, 7)
    for n in (2, 5, 64, 4096):
        f = np.float32(n) / np.float32(n - 1)
        var = (S * f).astype(np.float32)                    # vr_variance's formation
        assert np.array_equal(ha.tile_error(mu, S, n).view(np.uint32), ha.tile_error(mu, var, n, from_variance=True).view(np.uint32))


def test_schedule_functions():
    assert [ha.next_count(n, 64) for n in (2, 4, 16, 31, 32, 33, 63)] == [4, 8, 32, 62, 64, 64, 64]
    assert ha.next_count(2 ** 30 + 5, 2 ** 31 - 1) == 2 ** 31 - 1            # no overflow
    assert ha.next_count(3, 1000) == 6
    assert ha.converged(0.0999, 0.1) and not ha.converged(0.1, 0.1)           # strict
    assert not ha.converged(0.0, 0.0) and not ha.converged(float("nan"), 1.0) and not ha.converged(float("inf"), 1e30)
    counts = np.array([16, 4, 8, 4, 16, 64, 8], np.int32)
    assert ha.groups([6, 0, 1, 2, 3, 4], counts) == [(4, [1, 3]), (8, [6, 2]), (16, [0, 4])]
    assert ha.groups([], counts) == []


def test_schedule_replay_doubles_and_retires():
    # tile t converges once its count reaches conv[t]
    conv = [4, 8, 16, 10 ** 9, 32]
    err = lambda t, n: 0.0 if n >= conv[t] else 1.0      # noqa: E731
    n, rounds, hist = ha.replay(err, [0] * 5, list(range(5)), 4, 64, 0.5)
    assert list(n) == [4, 8, 16, 64, 32]
    assert rounds == 4                                      # evaluations at 4, 8, 16, 32; tile 3 at 64 is not evaluated again
    assert hist[0] == [(4, [1, 2, 3, 4])]
    n2, _, hist2 = ha.replay(err, [2, 8, 8, 40, 0], [0, 1, 3], 8, 64, 0.5)     # a subset of a ragged frame: several groups in one round
    assert list(n2) == [8, 8, 8, 64, 0]
    assert hist2[0] == [(40, [3])]
