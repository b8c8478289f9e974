"""ctypes binding of tests/hostkernel/libdemod_host.so: the albedo demodulation of the scattered layer (volren_amd/csrc/vr_demod.h) built for the host; replays
of RendererHIP::denoise / denoise_temporal / upsample with "denoise_layers" = 1 and "denoise_demodulate" = 1 on top of it and of the host builds of the filter,
the regression, the temporal passes and the upsampling's guide (hk_denoise, hk_regress, hk_temporal, hk_moments, hk_upsample); plus a float64 numpy statement
of the header, written from its text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_denoise
import hk_layers
import hk_moments
import hk_regress
import hk_temporal
import hk_upsample
from hk_common import _f32, _p

_lib = None
FLOOR = 2.0 ** -6


def build():
    return hk_common.build(__file__, "demod_host.cpp", "libdemod_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hk_demod_floor.restype = C.c_float
    return _lib


def floor():
    return float(lib().hk_demod_floor())


def divisor(feat):
    """feat [H][W][8] -> d [H][W][3] float32"""
    h, w = feat.shape[:2]
    d = np.zeros((h, w, 3), np.float32)
    lib().hk_demod_divisor(w * h, _p(_f32(feat, (h, w, 8))), _p(d))
    return d


def split(y, B, feat):
    """y, B [H][W][4], feat [H][W][8] -> S [H][W][4] float32."""
    h, w = y.shape[:2]
    S = np.zeros((h, w, 4), np.float32)
    lib().hk_demod_split(w * h, _p(_f32(y, (h, w, 4))), _p(_f32(B, (h, w, 4))), _p(_f32(feat, (h, w, 8))), _p(S))
    return S


def variance(var, feat, n):
    """prepare's v of the demodulated layer: var [H][W][4] unbiased variances, n the sample count or [H][W] counts -> v [H][W] float32"""
    h, w = var.shape[:2]
    v = np.zeros((h, w), np.float32)
    counts = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (h, w)))
    lib().hk_demod_variance(w * h, _p(_f32(var, (h, w, 4))), _p(_f32(feat, (h, w, 8))), _p(counts), _p(v))
    return v


def merge(F, B, feat):
    """F, B [H][W][4], feat [H][W][8] -> (out, L), [H][W][4] float32 each."""
    h, w = F.shape[:2]
    out, L = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    lib().hk_demod_merge(w * h, _p(_f32(F, (h, w, 4))), _p(_f32(B, (h, w, 4))), _p(_f32(feat, (h, w, 8))), _p(out), _p(L))
    return out, L


def upsample(L, glo, ghi, B, f, sigma=hk_denoise.DEFAULT_SIGMA, staged=False):
    """hk_upsample.upsample with the taps demodulated by the lo guide and the hi layer remodulated by the hi guide.  staged: the lo layer divided once per
    texel in front of plain taps, as the kernel's window holds it (the same values)"""
    h, w = L.shape[:2]
    H, W = f * h, f * w
    out, Lh = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    s = np.asarray(sigma, np.float32)
    lib().hk_demod_upsample(w, h, int(f), int(staged), _p(_f32(L, (h, w, 4))), _p(_f32(glo, (h, w, 8))), _p(_f32(ghi, (H, W, 8))), _p(_f32(B, (H, W, 4))), _p(s),
                            _p(out), _p(Lh))
    return out, Lh


def chain(L, feat_lo, o_hi, rays, f, sigma=hk_denoise.DEFAULT_SIGMA):
    """RendererHIP::upsample with "denoise_demodulate" = 1 on the host -> (out, L_hi, hi features, B)."""
    feat, B = hk_upsample.hi_inputs(o_hi, rays)
    out, Lh = upsample(L, hk_upsample.guide(feat_lo), hk_upsample.guide(feat), B, f, sigma)
    return out, Lh, feat, B


def filtered(S, v, g, iterations, sigma, ridge=None):
    """the a-trous iterations from (S, v), or with a ridge the regression on S (iterations = 0: S itself)"""
    if ridge is not None:
        return hk_regress.regress(S, g, ridge, sigma) if iterations else S
    F = S
    for k in range(iterations):
        F, v = hk_denoise.atrous(F, v, g, 1 << k, sigma)
    return F


def layered(y, B, var, feat, n, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA, ridge=None):
    """RendererHIP::denoise with denoise_layers = 1 and denoise_demodulate = 1 from the resolved frame on.  ridge: "denoise_filter" = 1 with that ridge.
    n: the sample count, or [H][W] counts of a ragged frame.  -> (out, L, S, F)"""
    S = split(y, B, feat)
    g = hk_denoise.prepare(var, feat, 1)[1]
    F = filtered(S, variance(var, feat, n), g, iterations, sigma, ridge)
    out, L = merge(F, B, feat)
    return out, L, S, F


class Replay:
    """RendererHIP::denoise_temporal with denoise_layers = 1 and denoise_demodulate = 1 on the host: the history holds the demodulated layer.
    moments: "denoise_moments" = 1; ridge: "denoise_filter" = 1 with that ridge."""

    def __init__(self, moments=False, ridge=None):
        self.moments, self.ridge, self.hist, self.stat = moments, ridge, None, None

    def frame(self, cur, y, B, var, feat, n, alpha, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA, tau=0.0):
        """-> (history colour, V, N, out, L)"""
        S = split(y, B, feat)
        g = hk_denoise.prepare(var, feat, 1)[1]
        if self.moments:
            c, rec, mom = hk_moments.step(cur, S, g, alpha, sigma, self.hist)
            self.hist = (np.array(cur, np.float32), c, rec, mom)
        else:
            v = variance(var, feat, n)
            if tau > 0:
                c, rec, self.stat = hk_temporal.step_reject(cur, S, v, g[..., 3], g[..., 7], alpha, tau, self.hist)
            else:
                (c, rec), self.stat = hk_temporal.step(cur, S, v, g[..., 3], g[..., 7], alpha, self.hist), None
            self.hist = (np.array(cur, np.float32), c, rec)
        V, N = np.ascontiguousarray(rec[..., 0]), np.ascontiguousarray(rec[..., 1])
        out, L = merge(filtered(c, V, g, iterations, sigma, self.ridge), B, feat)
        return c, V, N, out, L


# ---- the float64 statement (vr_demod.h's header comment), written from the formulas, not from the C++ -------------------------------------------------
def spec_divisor(feat, floor=FLOOR):
    """d = max(albedo, floor) per channel where kappa > 0, 1 elsewhere: [H][W][3]"""
    f = np.asarray(feat, np.float64)
    return np.where((f[..., 3] > 0)[..., None], np.maximum(f[..., 0:3], floor), 1.0)


def spec_split(y, B, feat, floor=FLOOR):
    S = hk_layers.spec_split(y, B, np.asarray(feat)[..., 3])
    S[..., :3] /= spec_divisor(feat, floor)
    return S


def spec_variance(var, feat, n, floor=FLOOR):
    """(sum_c w_c sqrt(max(var_c, 0)) / d_c)^2 / n"""
    t = np.sqrt(np.maximum(np.asarray(var, np.float64)[..., :3], 0.0)) / spec_divisor(feat, floor)
    s = t @ np.array(hk_denoise.LUMA)
    return s * s / np.asarray(n, np.float64)


def spec_merge(F, B, feat, floor=FLOOR):
    """-> (out, L): vr_layers.h's L, its rgb times d; out.rgb = max(0, (1 - kappa) B + L.rgb)"""
    k = np.asarray(feat, np.float64)[..., 3]
    _, L = hk_layers.spec_merge(F, B, k)
    L[..., :3] *= spec_divisor(feat, floor)
    out = np.concatenate([np.maximum(0.0, (1.0 - k)[..., None] * np.asarray(B, np.float64)[..., :3] + L[..., :3]), k[..., None]], axis=2)
    return out, L


def spec_upsample(L, glo, ghi, B, f, sigma=hk_denoise.DEFAULT_SIGMA, floor=FLOOR):
    """vr_upsample.h's statement on L.rgb / d_lo, its hi layer times d_hi -> (out, L_hi)"""
    Ld = np.array(L, np.float64)
    Ld[..., :3] /= spec_divisor(glo, floor)
    _, Lh, _, _ = hk_upsample.spec_upsample(Ld, glo, ghi, B, f, sigma)
    Lh[..., :3] *= spec_divisor(ghi, floor)
    k = np.asarray(ghi, np.float64)[..., 3]
    out = np.concatenate([np.maximum(0.0, (1.0 - k)[..., None] * np.asarray(B, np.float64)[..., :3] + Lh[..., :3]), k[..., None]], axis=2)
    return out, Lh


# ---- the same pipeline with another floor (tests/test_demod_host.py's sweep; float32 numpy, not bit for bit the product's) --------------------------------
def layered_with_floor(y, B, var, feat, n, floor, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA, ridge=None):
    """layered() with the divisor's floor replaced: the division, the variance and the multiplication in float32 numpy around the host filter -> out"""
    k = np.ascontiguousarray(feat[..., 3])
    d = np.where((k > 0)[..., None], np.maximum(feat[..., 0:3], np.float32(floor)), np.float32(1)).astype(np.float32)
    S = hk_layers.split(y, B, k)
    S[..., :3] /= d
    t = np.sqrt(np.maximum(var[..., :3], 0)).astype(np.float32) / d
    s = (t @ np.array(hk_denoise.LUMA, np.float32)).astype(np.float32)
    v = (s * s / np.float32(n)).astype(np.float32)
    g = hk_denoise.prepare(var, feat, 1)[1]
    F = filtered(S, v, g, iterations, sigma, ridge)
    _, L = hk_layers.merge(F, B, k)
    L[..., :3] *= d
    out = np.maximum(((1 - k)[..., None] * B[..., :3]).astype(np.float32) + L[..., :3], 0)
    return out
