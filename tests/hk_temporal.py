"""ctypes binding of tests/hostkernel/libtemporal_host.so: the temporal accumulation of the product's lane code (vr_temporal.h) built for the host, without
its history rejection and with it (steps 2a, 3a, in the two passes the HIP kernels make); a replay of RendererHIP::denoise_temporal on top of it and of
the host build of the filter (hk_denoise); plus an independent float64 numpy statement of the reprojection, the tap rules, the blend, the rejection
statistic and the decision.  TEST HARNESS ONLY.

A camera is 13 float32: cam_pos (3), cam_transform (9, column-major), cam_z."""
import ctypes as C

import numpy as np

import hk_common
import hk_denoise
from hk_common import _f32, _p

_lib = {}

DEPTH_BOUND = 0.1
MIN_WEIGHT = 2.0 ** -10
MAX_LENGTH = 2.0 ** 20
VARIANCE_FLOOR = 1e-12
WINDOW = 2
NO_HISTORY = -1.0
TAU_MIN, TAU_MAX = 2.0 ** -10, 2.0 ** 20
LUMA = hk_denoise.LUMA                            # vr_math.h luma


def build(sanitize=False):
    return hk_common.build(__file__, "temporal_host.cpp", "libtemporal_host_san.so" if sanitize else "libtemporal_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage") +
                           (("-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-g") if sanitize else ()))


def lib(sanitize=False):
    """sanitize: the build with the undefined-behaviour sanitizer (a float -> int conversion out of range or a signed overflow aborts the process)"""
    if sanitize not in _lib:
        L = C.CDLL(build(sanitize))
        L.hk_temporal_cam_z.restype = C.c_float
        L.hk_temporal_cam_z.argtypes = [C.c_float]
        L.hk_temporal_step_checked.restype = L.hk_reject_step_checked.restype = C.c_longlong
        _lib[sanitize] = L
    return _lib[sanitize]


def constants():
    """(default alpha, smallest alpha, largest alpha, depth bound, smallest weight sum, longest history) of vr_temporal.h"""
    out = np.zeros(6, np.float32)
    lib().hk_temporal_constants(_p(out))
    return tuple(float(x) for x in out)


def reject_constants():
    """(smallest tau, largest tau, variance floor, window radius, the statistic of a pixel without history) of vr_temporal.h"""
    out = np.zeros(5, np.float32)
    lib().hk_reject_constants(_p(out))
    return tuple(float(x) for x in out)


def cam_z(fov_degree):
    return np.float32(lib().hk_temporal_cam_z(C.c_float(float(fov_degree))))


def camera(pos, transform, fov_degree=None, z=None):
    """13 float32 from cam_pos, the column-major cam_transform and either the field of view (degrees) or cam_z itself"""
    c = np.zeros(13, np.float32)
    c[0:3] = np.asarray(pos, np.float32)
    c[3:12] = np.asarray(transform, np.float32).reshape(9)
    c[12] = cam_z(fov_degree) if z is None else np.float32(z)
    return c


def reproject(cur, prev, k, d):
    """Host build of step 1 alone: k, d [H][W] -> (u, w, dprev [H][W] float32, ok [H][W] bool); u, w, dprev are 0 where not ok."""
    h, w = k.shape
    u, ww, dp = (np.zeros((h, w), np.float32) for _ in range(3))
    ok = np.zeros((h, w), np.int32)
    lib().hk_temporal_reproject(w, h, _p(_f32(cur, (13,))), _p(_f32(prev, (13,))), _p(_f32(k, (h, w))), _p(_f32(d, (h, w))), _p(u), _p(ww), _p(dp), _p(ok))
    return u, ww, dp, ok != 0


def _step(name, cur, color, v, k, d, alpha, hist, checked, tau=None):
    """the call both steps share; T stays 0 without tau"""
    h, w = v.shape
    fn = getattr(lib(checked), name + ("_checked" if checked else ""))
    cur = _f32(cur, (13,))
    oc = np.zeros((h, w, 4), np.float32)
    orec = np.zeros((h, w, 4), np.float32)
    stat = np.zeros((h, w), np.float32)
    if hist is None:
        prev, hc, hr, have, same = cur, oc, orec, 0, 0
    else:
        prev, hc, hr = _f32(hist[0], (13,)), _f32(hist[1], (h, w, 4)), _f32(hist[2], (h, w, 4))
        have, same = 1, int(prev.tobytes() == cur.tobytes())
    args = [w, h, have, same, _p(cur), _p(prev), _p(_f32(color, (h, w, 4))), _p(_f32(v, (h, w))), _p(_f32(k, (h, w))), _p(_f32(d, (h, w))),
            _p(hc), _p(hr), C.c_float(float(alpha)), _p(oc), _p(orec)]
    if tau is not None:                                 # hk_reject_step: tau after alpha, T at the end
        args[13:13] = [C.c_float(float(tau))]
        args.append(_p(stat))
    bad = fn(*args)
    assert not checked or bad == 0, "%d reads outside the frame" % bad
    return oc, orec, stat


def step(cur, color, v, k, d, alpha, hist=None, checked=False):
    """Host build of steps 1-4 on a whole frame.  hist: None or (camera, colour [H][W][4], record [H][W][4] = (V, N, K, D)).  Whether the camera is
    unchanged is decided as the renderer decides it: the 13 floats byte for byte.  -> (colour, record) of the new history.
    checked: run the sanitizer build with every history read behind a range check; asserts that none fell outside the frame."""
    return _step("hk_temporal_step", cur, color, v, k, d, alpha, hist, checked)[:2]


def step_reject(cur, color, v, k, d, alpha, tau, hist=None, checked=False):
    """The same with steps 2a and 3a, tau > 0.  -> (colour, record, T [H][W]) of the new history.  checked: the window's reads are range-checked too."""
    assert tau > 0
    return _step("hk_reject_step", cur, color, v, k, d, alpha, hist, checked, tau)


def rejected(stat, tau):
    """the pixels with a history that step 3a rejected: not (T <= tau)"""
    with np.errstate(invalid="ignore"):
        return (stat != np.float32(NO_HISTORY)) & ~(stat <= np.float32(tau))


class Replay:
    """RendererHIP::denoise_temporal on the host: prepare (hk_denoise / hk_adaptive), the temporal step, the iterations."""

    def __init__(self):
        self.hist = None
        self.stat = None                              # T of the last frame; None after a frame with tau = 0

    def frame(self, cur, color, var, feat, n, alpha, iterations=5, sigma=hk_denoise.DEFAULT_SIGMA, tau=0.0):
        """n: the frame's sample count, or [H][W] counts of a ragged frame; tau: `denoise_reject`.  -> (history colour, V, N, denoised)"""
        if np.ndim(n) == 0:
            v, g = hk_denoise.prepare(var, feat, n)
        else:
            import hk_adaptive
            v, g = hk_adaptive.prepare(var, feat, n)
        if tau > 0:
            c, rec, self.stat = step_reject(cur, color, v, g[..., 3], g[..., 7], alpha, tau, self.hist)
        else:
            (c, rec), self.stat = step(cur, color, v, g[..., 3], g[..., 7], alpha, self.hist), None
        self.hist = (np.array(cur, np.float32), c, rec)
        out, vv = c, np.ascontiguousarray(rec[..., 0])
        for k in range(iterations):
            out, vv = hk_denoise.atrous(out, vv, g, 1 << k, sigma)
        return c, np.ascontiguousarray(rec[..., 0]), np.ascontiguousarray(rec[..., 1]), out


# ---- float64 statement of steps 1-4 (vr_temporal.h's header comment), written from the formulas, not from the C++ -------------------------------
def _unit(a):
    return a / np.sqrt((a * a).sum(axis=-1, keepdims=True))


def spec_reproject(cur, prev, k, d, dtype=np.float64):
    """-> (u, w, dprev, front): float arrays [H][W]; front = q.z < 0.  Values where not front are meaningless."""
    cur = np.asarray(cur, dtype)
    prev = np.asarray(prev, dtype)
    k = np.asarray(k, dtype)
    d = np.asarray(d, dtype)
    H, W = k.shape
    half = dtype(0.5)
    px, py = np.meshgrid(np.arange(W, dtype=dtype), np.arange(H, dtype=dtype))
    f = np.stack([((px + half) - dtype(W) * half) / dtype(H), ((py + half) - dtype(H) * half) / dtype(H), np.full((H, W), cur[12], dtype)], axis=-1)
    M = cur[3:12].reshape(3, 3).T                       # column-major: M[i][j] = m[3 j + i]
    Mp = prev[3:12].reshape(3, 3).T
    direction = _unit(_unit(f) @ M.T)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        X = cur[0:3] + d[..., None] * direction
        r = np.where((k > 0)[..., None], X - prev[0:3], direction)
        dprev = np.sqrt((r * r).sum(axis=-1))
        q = r @ Mp                                        # M'^T r
        s = prev[12] / q[..., 2]
        u = (q[..., 0] * s) * dtype(H) + dtype(W) * half - half
        w = (q[..., 1] * s) * dtype(H) + dtype(H) * half - half
    return u, w, dprev, q[..., 2] < 0


def spec_step(cur, color, v, k, d, alpha, hist=None, given=None):
    """float64 statement of steps 1-4.  hist as for step().  -> (C [H][W][4], V, N [H][W], u, w [H][W] (NaN without reprojection),
    ratio [H][W][4]: |D_q - d'| / max(D_q, d') of the four taps, NaN where it does not matter, sum_b [H][W]: the weight of the taps that count).
    given: (u, w, dprev, front) to use in place of step 1 (reproject()'s answer: steps 2-4 alone, from the coordinates the host build found)"""
    c = np.asarray(color, np.float64)
    v = np.asarray(v, np.float64)
    k = np.asarray(k, np.float64)
    d = np.asarray(d, np.float64)
    H, W = v.shape
    nan = np.full((H, W), np.nan)
    if hist is None:
        return c.copy(), v.copy(), np.ones((H, W)), nan, nan, np.full((H, W, 4), np.nan), np.zeros((H, W))
    prev = np.asarray(hist[0], np.float32)
    hc = np.asarray(hist[1], np.float64)
    rec = np.asarray(hist[2], np.float64)
    same = prev.tobytes() == np.asarray(cur, np.float32).tobytes()
    px, py = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    if same:
        u, w, dprev, front = px, py, d, np.ones((H, W), bool)
    elif given is not None:
        u, w, dprev = (np.asarray(a, np.float64) for a in given[:3])
        front = np.asarray(given[3], bool)
    else:
        u, w, dprev, front = spec_reproject(np.asarray(cur, np.float64), prev.astype(np.float64), k, d)
    C_out, V_out, N_out = c.copy(), v.copy(), np.ones((H, W))
    ratios = np.full((H, W, 4), np.nan)
    sum_b = np.zeros((H, W))
    for y in range(H):
        for x in range(W):
            if not front[y, x] or not np.isfinite(u[y, x]) or not np.isfinite(w[y, x]):
                continue
            x0, y0 = np.floor(u[y, x]), np.floor(w[y, x])
            ax, ay = u[y, x] - x0, w[y, x] - y0
            sb, sc, sv, nh = 0.0, np.zeros(4), 0.0, None
            t = -1
            for dy in (0, 1):
                for dx in (0, 1):
                    t += 1
                    xq, yq = x0 + dx, y0 + dy
                    if not (0 <= xq < W and 0 <= yq < H):
                        continue
                    xq, yq = int(xq), int(yq)
                    b = (ax if dx else 1.0 - ax) * (ay if dy else 1.0 - ay)
                    Vq, Nq, Kq, Dq = rec[yq, xq]
                    if not (b > 0 and Nq >= 1):
                        continue
                    if k[y, x] > 0:
                        with np.errstate(invalid="ignore", divide="ignore"):
                            ratios[y, x, t] = abs(Dq - dprev[y, x]) / max(Dq, dprev[y, x]) if Kq > 0 else np.nan
                        good = Kq > 0 and abs(Dq - dprev[y, x]) <= DEPTH_BOUND * max(Dq, dprev[y, x])
                    else:
                        good = k[y, x] == 0 and Kq == 0
                    if not good:
                        continue
                    sb += b
                    sc += b * hc[yq, xq]
                    sv += b * Vq
                    nh = Nq if nh is None else min(nh, Nq)
            sum_b[y, x] = sb
            if nh is None or sb < MIN_WEIGHT:
                continue
            N = min(nh + 1.0, MAX_LENGTH)
            a = max(float(alpha), 1.0 / N)
            C_out[y, x] = (1.0 - a) * (sc / sb) + a * c[y, x]
            V_out[y, x] = (1.0 - a) ** 2 * (sv / sb) + a * a * v[y, x]
            N_out[y, x] = N
    if same:
        u, w = nan, nan
    return C_out, V_out, N_out, u, w, ratios, sum_b


# ---- float64 statement of steps 2a and 3a, written from the formulas -----------------------------------------------------------------------------
def spec_fetch(cur, k, d, hist, given=None):
    """float64 (has [H][W], h [H][W][4], v_h, N_h [H][W]) of steps 1-3.  The fetch is spec_step's, so the statement is spec_step:
    blended with a frame of zeros at an alpha below every 1 / N it returns C = (1 - 1 / N) h, V = (1 - 1 / N)^2 v_h and N = N_h + 1 >= 2 where the pixel
    has a history, and N = 1 where it has none.  (Histories in the tests are shorter than 2^20 - 1 frames, where N stops counting.)"""
    H, W = np.shape(k)
    C_, V_, N_ = spec_step(cur, np.zeros((H, W, 4)), np.zeros((H, W)), k, d, 2.0 ** -40, hist, given=given)[:3]
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
