"""ctypes binding of tests/hostkernel/libupsample_host.so: the upsampling of the scattered layer (volren_amd/csrc/vr_upsample.h) and the window its kernel
stages (vr_tiles.h ScaledTileWindow) built for the host; the host chain of RendererHIP::upsample on top of it and of the host builds of the expected-value
pass and of resolve's background (hk_expected, hk_resolve); plus a float64 numpy statement of the header, written from its text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_denoise
import hk_expected
import hk_resolve
from hk_common import _f32, _p

_lib = None
MIN_WEIGHT = 2.0 ** -20


def build():
    return hk_common.build(__file__, "upsample_host.cpp", "libupsample_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hk_upsample_min_weight.restype = C.c_float
        _lib.hk_upsample_edge.restype = C.c_float
    return _lib


def min_weight():
    return float(lib().hk_upsample_min_weight())


def guide(features):
    """vr_denoise.h's guide of a feature buffer [H][W][8]: the same layout with the normal normalised, float32."""
    f = np.ascontiguousarray(features, np.float32)
    g = np.zeros_like(f)
    lib().hk_upsample_guide(f.size // 8, _p(f), _p(g))
    return g


def upsample(L, glo, ghi, B, f, sigma=hk_denoise.DEFAULT_SIGMA):
    """L [h][w][4] the lo layer, glo [h][w][8] the lo guide, ghi [H][W][8] the hi guide, B [H][W][4] the hi background -> (out, L_hi), [H][W][4] float32 each."""
    h, w = L.shape[:2]
    H, W = f * h, f * w
    out, Lh = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    s = np.asarray(sigma, np.float32)
    lib().hk_upsample(w, h, int(f), _p(_f32(L, (h, w, 4))), _p(_f32(glo, (h, w, 8))), _p(_f32(ghi, (H, W, 8))), _p(_f32(B, (H, W, 4))), _p(s), _p(out), _p(Lh))
    return out, Lh


def hi_inputs(o_hi, rays):
    """What RendererHIP::upsample forms at the hi size, on an oracle.binding.OracleRenderer of that size: (the expected-value feature buffer, B)."""
    feat = hk_expected.expected_pass(o_hi, rays)
    B, _ = hk_resolve.prepare(o_hi, rays, np.zeros((o_hi.h, o_hi.w, 4), np.float32))
    return feat, B


def chain(L, feat_lo, o_hi, rays, f, sigma=hk_denoise.DEFAULT_SIGMA):
    """RendererHIP::upsample on the host: L the lo layer, feat_lo the lo feature buffer, o_hi the scene at the hi size -> (out, L_hi, hi features, B)."""
    feat, B = hi_inputs(o_hi, rays)
    out, Lh = upsample(L, guide(feat_lo), guide(feat), B, f, sigma)
    return out, Lh, feat, B


def axis(x, f):
    """(x0, r, a, b[4]) of hi coordinate x as the lane code forms them"""
    xr, a, b = np.zeros(2, np.int32), C.c_float(), np.zeros(4, np.float32)
    lib().hk_upsample_axis(int(x), int(f), _p(xr), C.byref(a), _p(b))
    return int(xr[0]), int(xr[1]), np.float32(a.value), b


def edge(gp, gq, sigma=hk_denoise.DEFAULT_SIGMA):
    return np.float32(lib().hk_upsample_edge(_p(_f32(gp, (8,))), _p(_f32(gq, (8,))), _p(np.asarray(sigma, np.float32))))


def window(f, tile, W):
    """ScaledTileWindow<f> of hi tile `tile` of a hi frame W wide: (kFoot, kTexels, x0, y0) and first[256], the window index of every thread's first tap"""
    geom, at = np.zeros(4, np.int32), np.zeros(256, np.int32)
    assert lib().hk_upsample_window(int(f), int(tile), int(W), _p(geom), _p(at)) == 0, f
    return tuple(int(v) for v in geom), at


# ---- the float64 statement ----------------------------------------------------------------------------------------------------------------------------
def spec_spline(a):
    """the uniform cubic B-spline's four weights at fractions a: [..., 4]"""
    a = np.asarray(a, np.float64)
    return np.stack([(1 - a) ** 3, 3 * a ** 3 - 6 * a ** 2 + 4, -3 * a ** 3 + 3 * a ** 2 + 3 * a + 1, a ** 3], axis=-1) / 6.0


def spec_edge(gp, gq, sigma, coverage_weight=False):
    """vr_denoise.h's w_n w_d w_a between guides gp, gq [..., 8] in float64, 1 unless both coverages are positive; coverage_weight: times w_k everywhere"""
    sn, sd, sk, sa = (float(np.float32(sigma[i])) for i in (1, 2, 3, 4))
    gp, gq = np.asarray(gp, np.float64), np.asarray(gq, np.float64)
    both = (gp[..., 3] > 0) & (gq[..., 3] > 0)
    np_, nq = gp[..., 4:7], gq[..., 4:7]
    flat = ~np_.any(axis=-1) | ~nq.any(axis=-1)
    d = np.clip((np_ * nq).sum(axis=-1), 0.0, 1.0)
    wn = np.where(flat, 1.0, d ** sn)
    wd = np.exp(-np.abs(gp[..., 7] - gq[..., 7]) / (sd * np.maximum(gp[..., 7], gq[..., 7]) + float(np.float32(1e-6))))
    da = gp[..., 0:3] - gq[..., 0:3]
    wa = np.exp(-(da * da).sum(axis=-1) / (sa * sa))
    e = np.where(both, wn * wd * wa, 1.0)
    if coverage_weight:
        e = e * np.exp(-np.abs(gp[..., 3] - gq[..., 3]) / sk)
    return e


def spec_upsample(L, glo, ghi, B, f, sigma=hk_denoise.DEFAULT_SIGMA, coverage_weight=False):
    """vr_upsample.h's header comment in float64.  -> (out [H][W][4], L_hi [H][W][4], D_e [H][W], D_s [H][W])"""
    L, glo, ghi, B = (np.asarray(a, np.float64) for a in (L, glo, ghi, B))
    h, w = L.shape[:2]
    H, W = f * h, f * w
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x0, y0 = np.floor_divide(2 * xs + 1 - f, 2 * f), np.floor_divide(2 * ys + 1 - f, 2 * f)
    bx = spec_spline((2 * xs + 1 - f - 2 * f * x0) / (2.0 * f))
    by = spec_spline((2 * ys + 1 - f - 2 * f * y0) / (2.0 * f))
    Ne, Ns, De, Ds = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
    for j in range(4):
        for i in range(4):
            lx, ly = x0 - 1 + i, y0 - 1 + j
            ok = (lx >= 0) & (lx < w) & (ly >= 0) & (ly < h)
            cx, cy = np.clip(lx, 0, w - 1), np.clip(ly, 0, h - 1)
            s = np.where(ok, bx[..., i] * by[..., j], 0.0)
            se = s * spec_edge(ghi, glo[cy, cx], sigma, coverage_weight)
            Lq = L[cy, cx]
            Ne += se[..., None] * Lq[..., :3]
            De += se * Lq[..., 3]
            Ns += s[..., None] * Lq[..., :3]
            Ds += s * Lq[..., 3]
    first, second = De > MIN_WEIGHT, Ds > MIN_WEIGHT
    Cc = np.where(first[..., None], Ne / np.where(first, De, 1.0)[..., None], np.where(second[..., None], Ns / np.where(second, Ds, 1.0)[..., None], 0.0))
    k = ghi[..., 3]
    Lh = np.concatenate([k[..., None] * Cc, k[..., None]], axis=2)
    out = np.concatenate([np.maximum(0.0, (1.0 - k)[..., None] * B[..., :3] + Lh[..., :3]), k[..., None]], axis=2)
    return out, Lh, De, Ds
