"""ctypes binding of tests/hostkernel/libregress_host.so: the one-pass local-regression filter (volren_amd/csrc/vr_regress.h) built for the host; a replay of
RendererHIP::denoise / denoise_temporal with "denoise_layers" = 1 and "denoise_filter" = 1 on top of it and of the host builds of the resolve, the split and
merge and the temporal passes (hk_resolve, hk_layers, hk_temporal, hk_moments); plus a float64 numpy statement of the filter, written from the header's text.
TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_denoise
import hk_layers
import hk_moments
import hk_temporal
from hk_common import _f32, _p

_lib = None
RADIUS, TERMS = 5, 8
MIN_WEIGHT = MIN_DEPTH = PIVOT_FLOOR = RIDGE_MIN = 2.0 ** -20
RIDGE_MAX = 2.0 ** 20
SPATIAL_SIGMA = 2.5


def build():
    return hk_common.build(__file__, "regress_host.cpp", "libregress_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def constants():
    """(radius, terms, smallest weight, smallest depth, pivot floor, smallest ridge, largest ridge, default ridge) of vr_regress.h"""
    out = np.zeros(8, np.float32)
    lib().hk_regress_constants(_p(out))
    return tuple(float(x) for x in out)


def default_ridge():
    return constants()[7]


def ridge_ok(v):
    return bool(lib().hk_regress_ridge_ok(C.c_float(float(v))))


def regress(S, guide, ridge, sigma=hk_denoise.DEFAULT_SIGMA):
    """Host build of the filter on a whole frame: S [H][W][4], guide [H][W][8] (hk_denoise.prepare's) -> F [H][W][4] float32."""
    h, w = S.shape[:2]
    F = np.zeros((h, w, 4), np.float32)
    lib().hk_regress(w, h, _p(_f32(S, (h, w, 4))), _p(_f32(guide, (h, w, 8))), _p(np.asarray(sigma, np.float32)), C.c_float(float(ridge)), _p(F))
    return F


def dropped(S, guide, ridge, sigma=hk_denoise.DEFAULT_SIGMA):
    """regress() with the header's own counter: (F, int32 [H][W]: how many columns regress_solve dropped at each pixel, -1 where the pixel never reaches the solve)"""
    h, w = S.shape[:2]
    F, n = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.int32)
    lib().hk_regress_dropped(w, h, _p(_f32(S, (h, w, 4))), _p(_f32(guide, (h, w, 8))), _p(np.asarray(sigma, np.float32)), C.c_float(float(ridge)), _p(F), _p(n))
    return F, n


def solve(A, b, floor):
    """Host build of regress_solve: A [8][8] (upper triangle), b [8][3] -> beta_0 [3]."""
    out = np.zeros(3, np.float32)
    lib().hk_regress_solve(_p(_f32(A, (TERMS, TERMS))), _p(_f32(b, (TERMS, 3))), C.c_float(float(floor)), _p(out))
    return out


def _guide(feat):
    """the guide of a feature buffer (prepare's; the variance plays no part)"""
    return hk_denoise.prepare(np.zeros(feat.shape[:2] + (4,), np.float32), feat, 1)[1]


def layered(y, B, feat, ridge, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA):
    """RendererHIP::denoise with denoise_layers = 1 and denoise_filter = 1 from the resolved frame on: split, the regression on S (iterations = 0: S itself),
    merge.  -> (out, L, S, F)"""
    kappa = np.ascontiguousarray(feat[..., 3])
    S = hk_layers.split(y, B, kappa)
    F = regress(S, _guide(feat), ridge, sigma) if iterations else S
    out, L = hk_layers.merge(F, B, kappa)
    return out, L, S, F


class Replay:
    """RendererHIP::denoise_temporal with denoise_layers = 1 and denoise_filter = 1 on the host.  moments: "denoise_moments" = 1."""

    def __init__(self, moments=False):
        self.inner = hk_moments.Replay() if moments else hk_temporal.Replay()
        self.moments = moments

    def frame(self, cur, y, B, var, feat, n, alpha, ridge, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA, tau=0.0):
        """-> (history colour, V, N, out, L)"""
        kappa = np.ascontiguousarray(feat[..., 3])
        S = hk_layers.split(y, B, kappa)
        if self.moments:
            c, V, N = self.inner.frame(cur, S, var, feat, n, alpha, 0, sigma)[:3]
        else:
            c, V, N = self.inner.frame(cur, S, var, feat, n, alpha, 0, sigma, tau)[:3]
        F = regress(c, _guide(feat), ridge, sigma) if iterations else c
        out, L = hk_layers.merge(F, B, kappa)
        return c, V, N, out, L


# ---- the float64 statement (vr_regress.h's header comment), written from the formulas, not from the C++ ----------------------------------------------------
def spec_sums(S, guide, sigma=hk_denoise.DEFAULT_SIGMA):
    """float64 normal equations of every pixel: (A [H][W][8][8] symmetric, b [H][W][8][3])"""
    _, sn, sd, _, sa = (float(x) for x in sigma)
    S, g = np.asarray(S, np.float64), np.asarray(guide, np.float64)
    h, w = S.shape[:2]
    kp, dp, ap, gp = g[..., 3], g[..., 7], g[..., 0:3], g[..., 4:7]
    gp0 = (gp == 0).all(axis=-1)
    rd = 1.0 / np.maximum(dp, MIN_DEPTH)
    A, b = np.zeros((h, w, TERMS, TERMS)), np.zeros((h, w, TERMS, 3))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                Sq, inside = hk_denoise._shift(S, dy, dx)
                gq, _ = hk_denoise._shift(g, dy, dx)
                counts = inside & (Sq[..., 3] > MIN_WEIGHT) & (gq[..., 3] > 0)
                u = np.exp(-(dx * dx + dy * dy) / (2.0 * SPATIAL_SIGMA ** 2))
                e = np.ones((h, w))
                if dx or dy:
                    nq = gq[..., 4:7]
                    d = np.minimum(1.0, np.maximum(0.0, (gp * nq).sum(axis=-1)))
                    wn = np.where(gp0 | (nq == 0).all(axis=-1), 1.0, np.where(d > 0, d, 0.0) ** sn)
                    wd = np.exp(-np.abs(dp - gq[..., 7]) / (sd * np.maximum(dp, gq[..., 7]) + 1e-6))
                    da = ap - gq[..., 0:3]
                    wa = np.exp(-(da * da).sum(axis=-1) / (sa * sa))
                    e = np.where((kp > 0) & (gq[..., 3] > 0), wn * wd * wa, 1.0)
                se = np.where(counts, u * e, 0.0)
                x = np.concatenate([np.ones((h, w, 1)), ((gq[..., 7] - dp) * rd)[..., None], gq[..., 4:7] - gp, gq[..., 0:3] - ap], axis=-1)
                x = np.where(counts[..., None], x, 0.0)
                wq = se * np.where(counts, Sq[..., 3], 0.0)
                t = se[..., None] * np.where(counts[..., None], Sq[..., :3], 0.0)
                A += wq[..., None, None] * x[..., :, None] * x[..., None, :]
                b += x[..., :, None] * t[..., None, :]
    return A, b


PIVOT_SHARE = 2.0 ** -12


def spec_solve(M, b, floor):
    """float64 beta_0 [..., 3] of M beta = b (M [..., 8][8] symmetric, ridged; b [..., 8][3]) by the header's elimination in the order 0 .. 7: column k > 0 is kept
    iff its pivot d_k > floor and d_k > 2^-12 a_k, a_k = M_kk before the elimination; a dropped column's coefficient is 0 and the others are fitted without it.
    -> (beta_0, share [..., 8] = d_k / a_k, kept [..., 8])"""
    M, b = np.array(M, np.float64), np.array(b, np.float64)
    n = TERMS
    a = np.stack([M[..., k, k] for k in range(n)], axis=-1)
    d, kept = np.zeros_like(a), np.ones(a.shape, bool)
    with np.errstate(all="ignore"):
        for k in range(n):
            d[..., k] = M[..., k, k]
            if k:
                kept[..., k] = (d[..., k] > floor) & (d[..., k] > PIVOT_SHARE * a[..., k])
            for i in range(k + 1, n):
                l = np.where(kept[..., k], M[..., k, i] / d[..., k], 0.0)
                for j in range(i, n):
                    M[..., i, j] = M[..., i, j] - l * M[..., k, j]
                b[..., i, :] = b[..., i, :] - l[..., None] * b[..., k, :]
                M[..., k, i] = l
        beta = np.zeros_like(b)
        for k in range(n - 1, -1, -1):
            v = b[..., k, :] / d[..., k, None]
            for i in range(k + 1, n):
                v = v - M[..., k, i, None] * beta[..., i, :]
            beta[..., k, :] = np.where(kept[..., k, None], v, 0.0)
        return beta[..., 0, :], d / a, kept


def spec(S, guide, ridge, sigma=hk_denoise.DEFAULT_SIGMA, detail=False):
    """float64 F [H][W][4]: kappa_p = 0 -> 0; A_00 <= 2^-20 -> rgb 0; ridge 0 -> b_0 / A_00; else beta_0 of (A + ridge A_00 diag(0, 1, .. 1)) beta = b by
    spec_solve.  In exact arithmetic no pivot falls below the ridge, so the floor drops nothing; a column that keeps no more than 2^-12 of its own diagonal is
    dropped.  detail: -> (F, share [H][W][8], kept [H][W][8]) -- a pixel with a share near 2^-12 may decide otherwise in float32."""
    A, b = spec_sums(S, guide, sigma)
    kp = np.asarray(guide, np.float64)[..., 3]
    a00 = A[..., 0, 0]
    live = (kp != 0) & (a00 > MIN_WEIGHT)
    safe = np.where(live, a00, 1.0)
    share, kept = np.ones(a00.shape + (TERMS,)), np.ones(a00.shape + (TERMS,), bool)
    if ridge == 0:
        Ct = b[..., 0, :] / safe[..., None]
    else:
        M = A + (float(ridge) * safe)[..., None, None] * np.diag([0.0] + [1.0] * (TERMS - 1))
        M = np.where(live[..., None, None], M, np.eye(TERMS))
        Ct, share, kept = spec_solve(M, b, PIVOT_FLOOR * float(ridge) * safe)
    F = np.zeros(S.shape[:2] + (4,))
    F[..., :3] = np.where(live[..., None], kp[..., None] * Ct, 0.0)
    F[..., 3] = kp
    return (F, share, kept) if detail else F
