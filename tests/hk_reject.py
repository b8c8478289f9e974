"""ctypes binding of tests/hostkernel/libreject_host.so: the temporal accumulation with its history rejection (vr_temporal.h steps 2a, 3a) built for
the host in the two passes the HIP kernels make, a replay of RendererHIP::denoise_temporal with `denoise_reject` on top of it, plus a float64 numpy
statement of the statistic and the decision.  TEST HARNESS ONLY.

Cameras, histories and records are hk_temporal's."""
import ctypes as C
import os
import subprocess

import numpy as np

import hk_binding
import hk_denoise
import hk_temporal as ht

_DIR = hk_binding._DIR
_lib = {}

VARIANCE_FLOOR = 1e-12
WINDOW = 2
NO_HISTORY = -1.0
TAU_MIN, TAU_MAX = 2.0 ** -10, 2.0 ** 20
LUMA = (0.212671, 0.715160, 0.072169)          # vr_math.h luma


def build(sanitize=False):
    so = os.path.join(_DIR, "libreject_host_san.so" if sanitize else "libreject_host.so")
    src = os.path.join(_DIR, "reject_host.cpp")
    deps = [src] + [os.path.join(hk_binding._ROOT, "volren_amd", "csrc", f) for f in ("vr_temporal.h", "vr_math.h")]
    if not (os.path.exists(so) and all(os.path.getmtime(d) <= os.path.getmtime(so) for d in deps)):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-mavx2",
               "-Wno-unknown-pragmas", "-Wno-subobject-linkage", "-o", so, src]
        if sanitize:
            cmd[1:1] = ["-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-g"]
        subprocess.check_call(cmd)
    return so


def lib(sanitize=False):
    """sanitize: the build with the undefined-behaviour sanitizer (a float -> int conversion out of range or a signed overflow aborts the process)"""
    if sanitize not in _lib:
        L = C.CDLL(build(sanitize))
        L.hk_reject_step_checked.restype = C.c_longlong
        _lib[sanitize] = L
    return _lib[sanitize]


_p, _f32 = ht._p, ht._f32


def constants():
    """(smallest tau, largest tau, variance floor, window radius, the statistic of a pixel without history) of vr_temporal.h"""
    out = np.zeros(5, np.float32)
    lib().hk_reject_constants(_p(out))
    return tuple(float(x) for x in out)


def step(cur, color, v, k, d, alpha, tau, hist=None, checked=False):
    """Host build of steps 1-4 with 2a and 3a on a whole frame, tau > 0; arguments as hk_temporal.step.  -> (colour, record, T [H][W]) of the new history.
    checked: the sanitizer build with every history and window read behind a range check; asserts that none fell outside the frame."""
    assert tau > 0
    h, w = v.shape
    fn = lib(True).hk_reject_step_checked if checked else lib().hk_reject_step
    cur = _f32(cur, (13,))
    oc = np.zeros((h, w, 4), np.float32)
    orec = np.zeros((h, w, 4), np.float32)
    stat = np.zeros((h, w), np.float32)
    if hist is None:
        prev, hc, hr, have, same = cur, oc, orec, 0, 0
    else:
        prev, hc, hr = _f32(hist[0], (13,)), _f32(hist[1], (h, w, 4)), _f32(hist[2], (h, w, 4))
        have, same = 1, int(prev.tobytes() == cur.tobytes())
    bad = fn(w, h, have, same, _p(cur), _p(prev), _p(_f32(color, (h, w, 4))), _p(_f32(v, (h, w))), _p(_f32(k, (h, w))), _p(_f32(d, (h, w))),
             _p(hc), _p(hr), C.c_float(float(alpha)), C.c_float(float(tau)), _p(oc), _p(orec), _p(stat))
    assert not checked or bad == 0, "%d reads outside the frame" % bad
    return oc, orec, stat


def rejected(stat, tau):
    """the pixels with a history that step 3a rejected: not (T <= tau)"""
    with np.errstate(invalid="ignore"):
        return (stat != np.float32(NO_HISTORY)) & ~(stat <= np.float32(tau))


class Replay:
    """RendererHIP::denoise_temporal on the host with `denoise_reject` = tau: prepare, the temporal step (hk_temporal's for tau = 0), the iterations."""

    def __init__(self):
        self.hist = None
        self.stat = None                              # T of the last frame; None after a frame with tau = 0

    def frame(self, cur, color, var, feat, n, alpha, tau, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA):
        """n: the frame's sample count, or [H][W] counts of a ragged frame.  -> (history colour, V, N, denoised)"""
        if np.ndim(n) == 0:
            v, g = hk_denoise.prepare(var, feat, n)
        else:
            import hk_adaptive
            v, g = hk_adaptive.prepare(var, feat, n)
        if tau > 0:
            c, rec, self.stat = step(cur, color, v, g[..., 3], g[..., 7], alpha, tau, self.hist)
        else:
            (c, rec), self.stat = ht.step(cur, color, v, g[..., 3], g[..., 7], alpha, self.hist), None
        self.hist = (np.array(cur, np.float32), c, rec)
        out, vv = c, np.ascontiguousarray(rec[..., 0])
        for k in range(iterations):
            out, vv = hk_denoise.atrous(out, vv, g, 1 << k, sigma)
        return c, np.ascontiguousarray(rec[..., 0]), np.ascontiguousarray(rec[..., 1]), out


# ---- float64 statement of steps 2a and 3a, written from the formulas -----------------------------------------------------------------------------
def spec_fetch(cur, k, d, hist, given=None):
    """float64 (has [H][W], h [H][W][4], v_h, N_h [H][W]) of steps 1-3.  The fetch is today's, so the statement is today's (hk_temporal.spec_step):
    blended with a frame of zeros at an alpha below every 1 / N it returns C = (1 - 1 / N) h, V = (1 - 1 / N)^2 v_h and N = N_h + 1 >= 2 where the pixel
    has a history, and N = 1 where it has none.  (Histories in the tests are shorter than 2^20 - 1 frames, where N stops counting.)"""
    H, W = np.shape(k)
    C_, V_, N_ = ht.spec_step(cur, np.zeros((H, W, 4)), np.zeros((H, W)), k, d, 2.0 ** -40, hist, given=given)[:3]
    has = N_ >= 2
    oma = np.where(has, 1.0 - 1.0 / N_, 1.0)
    return has, np.where(has[..., None], C_ / oma[..., None], 0.0), np.where(has, V_ / (oma * oma), 0.0), np.where(has, N_ - 1.0, 0.0)


def spec_stat(color, v, has, h, vh):
    """float64 T [H][W] (-1 without history) from the frame (colour [H][W][4], v) and the fetch"""
    c = np.asarray(color, np.float64)
    w = np.asarray(LUMA, np.float64)
    dl = (h[..., :3] * w).sum(axis=-1) - (c[..., :3] * w).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        z2 = np.where(has, dl * dl / ((np.asarray(v, np.float64) + vh) + VARIANCE_FLOOR), 0.0)
    H, W = has.shape
    zs = np.zeros((H + 2 * WINDOW, W + 2 * WINDOW))
    ns = np.zeros_like(zs)
    zs[WINDOW:WINDOW + H, WINDOW:WINDOW + W] = z2
    ns[WINDOW:WINDOW + H, WINDOW:WINDOW + W] = has
    total, count = np.zeros((H, W)), np.zeros((H, W))
    for dy in range(2 * WINDOW + 1):
        for dx in range(2 * WINDOW + 1):
            total += zs[dy:dy + H, dx:dx + W]
            count += ns[dy:dy + H, dx:dx + W]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(has, total / count, NO_HISTORY)
