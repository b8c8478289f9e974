"""ctypes binding of tests/hostkernel/libmoments_host.so: the temporal luminance moments of the product's lane code (vr_moments.h) built for the host, in
the two passes the HIP kernels make; a replay of RendererHIP::denoise_temporal with "denoise_moments" = 1 on top of it and of the host build of the
filter (hk_denoise); plus an independent float64 numpy statement of the fetch, the blend and the variance pass.  TEST HARNESS ONLY.

A camera is 13 float32: cam_pos (3), cam_transform (9, column-major), cam_z (hk_temporal.camera)."""
import ctypes as C

import numpy as np

import hk_common
import hk_denoise
import hk_temporal as ht
from hk_common import _f32, _p

_lib = None

MIN_LENGTH = 4.0
WINDOW = 3
OFF_FRAME = -1.0
LUMA = hk_denoise.LUMA


def build():
    return hk_common.build(__file__, "moments_host.cpp", "libmoments_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hk_moments_pass1.restype = _lib.hk_moments_pass2.restype = C.c_longlong
    return _lib


def constants():
    """(history length from which the temporal variance counts, window radius, the m2 word of a pixel off the frame) of vr_moments.h"""
    out = np.zeros(3, np.float32)
    lib().hk_moments_constants(_p(out))
    return tuple(float(x) for x in out)


def pass1(cur, color, k, d, alpha, hist=None, checked=False):
    """Host build of pass 1 on a whole frame.  hist: None or (camera, colour, record = (V, N, K, D), moments = (m1, m2, E, S)), each [H][W][4].
    -> (colour, record, moments) of the new history with V = 0 and S = 0.  checked: every history read behind a range check; asserts that none fell
    outside the frame."""
    h, w = k.shape
    cur = _f32(cur, (13,))
    oc, orec, om = (np.zeros((h, w, 4), np.float32) for _ in range(3))
    if hist is None:
        prev, hc, hr, hm, have, same = cur, oc, orec, om, 0, 0
    else:
        prev, hc, hr, hm = _f32(hist[0], (13,)), _f32(hist[1], (h, w, 4)), _f32(hist[2], (h, w, 4)), _f32(hist[3], (h, w, 4))
        have, same = 1, int(prev.tobytes() == cur.tobytes())
    bad = lib().hk_moments_pass1(int(checked), w, h, have, same, _p(cur), _p(prev), _p(_f32(color, (h, w, 4))), _p(_f32(k, (h, w))), _p(_f32(d, (h, w))),
                                 _p(hc), _p(hr), _p(hm), C.c_float(float(alpha)), _p(oc), _p(orec), _p(om))
    assert bad == 0, "%d history reads outside the frame" % bad
    return oc, orec, om


def pass2(guide, sigma, record, moments, checked=False):
    """Host build of pass 2 on pass 1's record and moments (not changed).  -> (record with V, moments with S, v [H][W])"""
    h, w = record.shape[:2]
    rec, mom = _f32(record, (h, w, 4)).copy(), _f32(moments, (h, w, 4)).copy()
    v = np.zeros((h, w), np.float32)
    s = np.asarray(sigma, np.float32)
    bad = lib().hk_moments_pass2(int(checked), w, h, _p(_f32(guide, (h, w, 8))), _p(s), _p(rec), _p(mom), _p(v))
    assert bad == 0, "%d window or guide reads outside the frame" % bad
    return rec, mom, v


def step(cur, color, guide, alpha, sigma=hk_denoise.DEFAULT_SIGMA, hist=None, checked=False):
    """Both passes.  guide [H][W][8] (hk_denoise.prepare's).  -> (colour, record, moments) of the new history"""
    c, rec, mom = pass1(cur, color, guide[..., 3], guide[..., 7], alpha, hist, checked)
    rec, mom, _ = pass2(guide, sigma, rec, mom, checked)
    return c, rec, mom


class Replay:
    """RendererHIP::denoise_temporal with denoise_moments = 1 on the host: prepare (for the guide), the two passes, the iterations."""

    def __init__(self):
        self.hist = None

    def frame(self, cur, color, var, feat, n, alpha, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA):
        """-> (history colour, V, N, moment records, denoised)"""
        _, g = hk_denoise.prepare(var, feat, n)
        c, rec, mom = step(cur, color, g, alpha, sigma, self.hist)
        self.hist = (np.array(cur, np.float32), c, rec, mom)
        out, vv = c, np.ascontiguousarray(rec[..., 0])
        for k in range(iterations):
            out, vv = hk_denoise.atrous(out, vv, g, 1 << k, sigma)
        return c, np.ascontiguousarray(rec[..., 0]), np.ascontiguousarray(rec[..., 1]), mom, out


# ---- float64 statement (vr_moments.h's header comment), written from the formulas, not from the C++ --------------------------------------------
def spec_pass1(cur, color, k, d, alpha, hist=None, given=None):
    """float64 (C [H][W][4], N, m1, m2, E [H][W], near [H][W]).  The fetch is hk_temporal.spec_fetch's -- the statement of vr_temporal.h's steps 1-3 --
    run once on the history's colours and once on its moment records in the colours' place: the same taps, the same weights.  near: a tap's depth
    ratio lies within 1e-5 of the bound, so float32 may weigh other taps.  given: hk_temporal.reproject's answer, in place of step 1."""
    c = np.asarray(color, np.float64)
    H, W = c.shape[:2]
    L = c[..., :3] @ np.asarray(LUMA, np.float64)
    if hist is None:
        return c.copy(), np.ones((H, W)), L, L * L, np.ones((H, W)), np.zeros((H, W), bool)
    cam, hc, rec, mom = hist
    has, h, _, nh = ht.spec_fetch(cur, k, d, (cam, hc, rec), given=given)
    _, hm, _, _ = ht.spec_fetch(cur, k, d, (cam, mom, rec), given=given)
    ratio = ht.spec_step(cur, np.zeros((H, W, 4)), np.zeros((H, W)), k, d, alpha, (cam, hc, rec), given=given)[5]
    with np.errstate(invalid="ignore"):
        near = (np.abs(ratio - ht.DEPTH_BOUND) <= 1e-5).any(axis=-1)
    N = np.where(has, np.minimum(nh + 1.0, ht.MAX_LENGTH), 1.0)
    a = np.maximum(float(alpha), 1.0 / N)
    oma = 1.0 - a
    C_ = np.where(has[..., None], oma[..., None] * h + a[..., None] * c, c)
    m1 = np.where(has, oma * hm[..., 0] + a * L, L)
    m2 = np.where(has, oma * hm[..., 1] + a * L * L, L * L)
    E = np.where(has, oma * oma * hm[..., 2] + a * a, 1.0)
    return C_, N, m1, m2, E, near


def spec_pass2(guide, sigma, N, m1, m2, E):
    """float64 (S, V, a2 [H][W]): a2 is the second moment S was formed from (m2 itself where N >= 4), the scale of S's rounding error."""
    sc, sn, sd, sk, sa = (float(x) for x in sigma)
    g = np.asarray(guide, np.float64)
    m1 = np.asarray(m1, np.float64)
    m2 = np.asarray(m2, np.float64)
    H, W = m1.shape
    kp, dp, ap, gp = g[..., 3], g[..., 7], g[..., 0:3], g[..., 4:7]
    gp0 = (gp == 0).all(axis=-1)
    sw, s1, s2 = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(invalid="ignore", divide="ignore"):
        for dy in range(-WINDOW, WINDOW + 1):
            for dx in range(-WINDOW, WINDOW + 1):
                q1, inside = hk_denoise._shift(m1, dy, dx)
                q2, _ = hk_denoise._shift(m2, dy, dx)
                gq, _ = hk_denoise._shift(g, dy, dx)
                wt = np.ones((H, W))
                if dx or dy:
                    wt = np.exp(-np.abs(kp - gq[..., 3]) / sk)
                    both = (kp > 0) & (gq[..., 3] > 0)
                    nq = gq[..., 4:7]
                    dot = np.minimum(1.0, np.maximum(0.0, (gp * nq).sum(axis=-1)))
                    wn = np.where(gp0 | (nq == 0).all(axis=-1), 1.0, np.where(dot > 0, dot, 0.0) ** sn)
                    wd = np.exp(-np.abs(dp - gq[..., 7]) / (sd * np.maximum(dp, gq[..., 7]) + 1e-6))
                    da = ap - gq[..., 0:3]
                    wa = np.exp(-(da * da).sum(axis=-1) / (sa * sa))
                    wt = np.where(both, wt * wn * wd * wa, wt)
                wt = np.where(inside, wt, 0.0)
                sw += wt
                s1 += np.where(inside, wt * q1, 0.0)
                s2 += np.where(inside, wt * q2, 0.0)
        a1, a2 = s1 / sw, s2 / sw
        long_ = np.asarray(N) >= MIN_LENGTH
        a1 = np.where(long_, m1, a1)
        a2 = np.where(long_, m2, a2)
        S = np.maximum(a2 - a1 * a1, 0.0)
    return S, S * np.asarray(E, np.float64), a2
