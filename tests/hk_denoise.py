"""ctypes binding of tests/hostkernel/libdenoise_host.so: the a-trous denoiser of the product's lane code (vr_denoise.h) built for the host, plus
an independent float64 numpy statement of the same filter.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
from hk_common import _f32, _p

_lib = None

DEFAULT_SIGMA = (4.0, 0.5, 0.1, 0.25, 0.2)          # colour, normal, depth, coverage, albedo
LUMA = (0.212671, 0.715160, 0.072169)
B3 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
G3 = (1 / 4, 1 / 2, 1 / 4)


def build():
    return hk_common.build(__file__, "denoise_host.cpp", "libdenoise_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def sigma_range():
    """(smallest, largest) value of each sigma that vr_set_float "denoise_sigma" accepts (vr_denoise.h kDenoiseSigmaMin / Max)"""
    r = np.zeros(2, np.float32)
    lib().hk_denoise_sigma_range(_p(r))
    return float(r[0]), float(r[1])


def denoise(color, var, feat, n, iterations=5, sigma=DEFAULT_SIGMA):
    """The host build of the whole filter: color / var [H][W][4], feat [H][W][8], n samples -> [H][W][4] float32."""
    h, w = color.shape[:2]
    c, v, f = _f32(color, (h, w, 4)), _f32(var, (h, w, 4)), _f32(feat, (h, w, 8))
    s = np.asarray(sigma, np.float32)
    out = np.zeros((h, w, 4), np.float32)
    lib().hk_denoise(w, h, int(n), _p(c), _p(v), _p(f), int(iterations), _p(s), _p(out))
    return out


def prepare(var, feat, n):
    """Host build of the prepare step: -> (v [H][W], guide [H][W][8])."""
    h, w = var.shape[:2]
    v = np.zeros((h, w), np.float32)
    g = np.zeros((h, w, 8), np.float32)
    lib().hk_denoise_prepare(w, h, int(n), _p(_f32(var, (h, w, 4))), _p(_f32(feat, (h, w, 8))), _p(v), _p(g))
    return v, g


def atrous(color, v, guide, step, sigma=DEFAULT_SIGMA):
    """Host build of one iteration: -> (colour [H][W][4], v [H][W])."""
    h, w = color.shape[:2]
    c2 = np.zeros((h, w, 4), np.float32)
    v2 = np.zeros((h, w), np.float32)
    s = np.asarray(sigma, np.float32)
    lib().hk_denoise_atrous(w, h, int(step), _p(_f32(color, (h, w, 4))), _p(_f32(v, (h, w))), _p(_f32(guide, (h, w, 8))), _p(s), _p(c2), _p(v2))
    return c2, v2


# ---- float64 statement of the filter (vr_denoise.h's header comment), written from the formulas, not from the C++ ----------------------------
def spec_prepare(var, feat, n):
    var = np.maximum(np.asarray(var, np.float64), 0.0)
    s = sum(LUMA[i] * np.sqrt(var[..., i]) for i in range(3))
    v = s * s / float(n)
    feat = np.asarray(feat, np.float64)
    g = feat.copy()
    nrm = feat[..., 4:7]
    ln = np.sqrt((nrm * nrm).sum(axis=-1, keepdims=True))
    g[..., 4:7] = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), 0.0)
    return v, g


def _shift(a, dy, dx, fill=0.0):
    """b[y, x] = a[y + dy, x + dx] where inside, `fill` elsewhere; and the mask of the inside."""
    h, w = a.shape[:2]
    b = np.full(a.shape, fill, np.float64)
    m = np.zeros((h, w), bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m[y0:y1, x0:x1] = True
    return b, m


def spec_atrous(color, v, guide, step, sigma=DEFAULT_SIGMA):
    sc, sn, sd, sk, sa = (float(x) for x in sigma)
    c = np.asarray(color, np.float64)
    v = np.asarray(v, np.float64)
    g = np.asarray(guide, np.float64)
    h, w = v.shape
    vs = np.zeros((h, w))
    ws = np.zeros((h, w))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            vq, m = _shift(v, dy, dx)
            k = G3[dx + 1] * G3[dy + 1]
            vs += np.where(m, k * vq, 0.0)
            ws += np.where(m, k, 0.0)
    vbar = vs / ws
    L = c[..., :3] @ np.array(LUMA)
    dc = sc * np.sqrt(vbar) + 1e-6
    kp, dp, ap, gp = g[..., 3], g[..., 7], g[..., 0:3], g[..., 4:7]
    gp0 = (gp == 0).all(axis=-1)
    acc = np.zeros((h, w, 4))
    sw = np.zeros((h, w))
    sv = np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cq, m = _shift(c, step * dy, step * dx)
            vq, _ = _shift(v, step * dy, step * dx)
            gq, _ = _shift(g, step * dy, step * dx)
            wt = np.full((h, w), B3[dx + 2] * B3[dy + 2])
            if dx or dy:
                Lq = cq[..., :3] @ np.array(LUMA)
                wt = wt * np.exp(-np.abs(L - Lq) / dc) * np.exp(-np.abs(kp - gq[..., 3]) / sk)
                both = (kp > 0) & (gq[..., 3] > 0)
                nq = gq[..., 4:7]
                d = np.minimum(1.0, np.maximum(0.0, (gp * nq).sum(axis=-1)))
                wn = np.where(gp0 | (nq == 0).all(axis=-1), 1.0, np.where(d > 0, d, 0.0) ** sn)
                wd = np.exp(-np.abs(dp - gq[..., 7]) / (sd * np.maximum(dp, gq[..., 7]) + 1e-6))
                da = ap - gq[..., 0:3]
                wa = np.exp(-(da * da).sum(axis=-1) / (sa * sa))
                wt = np.where(both, wt * wn * wd * wa, wt)
            wt = np.where(m, wt, 0.0)
            acc += wt[..., None] * cq
            sw += wt
            sv += wt * wt * vq
    return acc / sw[..., None], sv / (sw * sw)


def spec_denoise(color, var, feat, n, iterations=5, sigma=DEFAULT_SIGMA):
    v, g = spec_prepare(var, feat, n)
    c = np.asarray(color, np.float64)
    for k in range(iterations):
        c, v = spec_atrous(c, v, g, 1 << k, sigma)
    return c
