"""ctypes binding of tests/hostkernel/liblayers_host.so: the split and merge of the layered filter (volren_amd/csrc/vr_layers.h) built for the host; a
replay of RendererHIP::denoise / denoise_temporal with "denoise_layers" = 1 on top of them and of the host builds of the resolve, the filter and the
temporal passes (hk_resolve, hk_denoise, hk_temporal, hk_moments); plus a float64 numpy statement of the split and the merge, written from the header's
text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_denoise
import hk_moments
import hk_resolve
import hk_temporal
from hk_common import _f32, _p

_lib = None
MIN_WEIGHT = 2.0 ** -20


def build():
    return hk_common.build(__file__, "layers_host.cpp", "liblayers_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hk_layers_min_weight.restype = C.c_float
    return _lib


def min_weight():
    return float(lib().hk_layers_min_weight())


def split(y, B, kappa):
    """y, B [H][W][4], kappa [H][W] -> S [H][W][4] float32."""
    h, w = y.shape[:2]
    S = np.zeros((h, w, 4), np.float32)
    lib().hk_layers_split(w * h, _p(_f32(y, (h, w, 4))), _p(_f32(B, (h, w, 4))), _p(_f32(kappa, (h, w))), _p(S))
    return S


def merge(F, B, kappa):
    """F, B [H][W][4], kappa [H][W] -> (out, L), [H][W][4] float32 each."""
    h, w = F.shape[:2]
    out, L = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    lib().hk_layers_merge(w * h, _p(_f32(F, (h, w, 4))), _p(_f32(B, (h, w, 4))), _p(_f32(kappa, (h, w))), _p(out), _p(L))
    return out, L


def layered(y, B, var, guide, n, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA):
    """RendererHIP::denoise with denoise_layers = 1 from the resolved frame on: split, the host filter on S with the frame's variance, merge.
    n: the sample count, or [H][W] counts of a ragged frame.  -> (out, L, S, F)"""
    kappa = np.ascontiguousarray(guide[..., 3])
    S = split(y, B, kappa)
    if np.ndim(n) == 0:
        F = hk_denoise.denoise(S, var, guide, n, iterations, sigma)
    else:
        import hk_adaptive
        v, g = hk_adaptive.prepare(var, guide, n)
        F = S
        for k in range(iterations):
            F, v = hk_denoise.atrous(F, v, g, 1 << k, sigma)
    out, L = merge(F, B, kappa)
    return out, L, S, F


def denoise(o, rays, fb, var, guide, n, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA):
    """The whole call on an oracle.binding.OracleRenderer's scene: resolve (hk_resolve), then layered().  -> (out, L, y)"""
    y, B = hk_resolve.resolved(o, rays, fb, guide)
    out, L, _, _ = layered(y, B, var, guide, n, iterations, sigma)
    return out, L, y


class Replay:
    """RendererHIP::denoise_temporal with denoise_layers = 1 on the host: the history holds the layer.  moments: "denoise_moments" = 1."""

    def __init__(self, moments=False):
        self.inner = hk_moments.Replay() if moments else hk_temporal.Replay()
        self.moments = moments

    def frame(self, cur, y, B, var, guide, n, alpha, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA, tau=0.0):
        """-> (history colour, V, N, out, L)"""
        kappa = np.ascontiguousarray(guide[..., 3])
        S = split(y, B, kappa)
        if self.moments:
            c, V, N, _, F = self.inner.frame(cur, S, var, guide, n, alpha, iterations, sigma)
        else:
            c, V, N, F = self.inner.frame(cur, S, var, guide, n, alpha, iterations, sigma, tau)
        out, L = merge(F, B, kappa)
        return c, V, N, out, L


# ---- the float64 statement ----------------------------------------------------------------------------------------------------------------------------
def spec_split(y, B, kappa):
    """vr_layers.h's header comment in float64: S.rgb = y.rgb - (1 - kappa) B, S.a = kappa."""
    y, B, k = np.asarray(y, np.float64), np.asarray(B, np.float64)[..., :3], np.asarray(kappa, np.float64)
    return np.concatenate([y[..., :3] - (1.0 - k)[..., None] * B, k[..., None]], axis=2)


def spec_merge(F, B, kappa):
    """-> (out, L): L.rgb = F.rgb kappa / F.a where F.a > 2^-20, else F.rgb; out.rgb = max(0, (1 - kappa) B + L.rgb); both alphas kappa."""
    F, B, k = np.asarray(F, np.float64), np.asarray(B, np.float64)[..., :3], np.asarray(kappa, np.float64)
    big = F[..., 3] > MIN_WEIGHT
    r = np.where(big, k / np.where(big, F[..., 3], 1.0), 1.0)
    L = np.concatenate([F[..., :3] * r[..., None], k[..., None]], axis=2)
    out = np.concatenate([np.maximum(0.0, (1.0 - k)[..., None] * B + L[..., :3]), k[..., None]], axis=2)
    return out, L
