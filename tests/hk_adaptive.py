"""ctypes binding of tests/hostkernel/libadaptive_host.so: the adaptive-sampling lane code of the product (vr_adaptive.h) built for the host, plus an
independent float64 numpy statement of the error estimate and a replay of the schedule.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
from hk_common import _f32, _p

_lib = None

LUMA = (0.212671, 0.715160, 0.072169)
FLOOR = 2.0 ** -10


def build():
    return hk_common.build(__file__, "adaptive_host.cpp", "libadaptive_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_adaptive_next_count.restype = C.c_int
        L.hk_adaptive_next_count.argtypes = [C.c_int, C.c_int]
        L.hk_adaptive_converged.restype = C.c_int
        L.hk_adaptive_converged.argtypes = [C.c_float, C.c_float]
        L.hk_adaptive_floor.restype = C.c_float
        L.hk_adaptive_groups.restype = C.c_int
        _lib = L
    return _lib


def tiles_of(w, h):
    return (h + 15) // 16, (w + 15) // 16


def per_pixel(counts, w, h):
    """[tiles_y][tiles_x] counts -> [H][W] counts of the pixels"""
    c = np.asarray(counts).reshape(tiles_of(w, h))
    return np.ascontiguousarray(np.repeat(np.repeat(c, 16, axis=0), 16, axis=1)[:h, :w], np.int32)


def pixel_error(mu, S, n):
    """host build of e_p: mu, S [...][4], n [...] -> float32 [...]"""
    mu = np.ascontiguousarray(mu, np.float32)
    S = np.ascontiguousarray(S, np.float32)
    n = np.ascontiguousarray(np.broadcast_to(n, mu.shape[:-1]), np.int32)
    e = np.zeros(mu.shape[:-1], np.float32)
    lib().hk_adaptive_pixel_error(int(n.size), _p(mu), _p(S), _p(n), _p(e))
    return e


def tile_error(mu, S, counts, from_variance=False):
    """host build of e_t: mu / S [H][W][4] (framebuffer, moments -- or, from_variance, the variance as vr_variance returns it), counts
    [tiles_y][tiles_x] (or a scalar) -> float32 [tiles_y][tiles_x]"""
    h, w = mu.shape[:2]
    ty, tx = tiles_of(w, h)
    c = np.ascontiguousarray(np.broadcast_to(np.asarray(counts, np.int32), (ty, tx)), np.int32)
    e = np.zeros((ty, tx), np.float32)
    lib().hk_adaptive_tile_error(w, h, _p(_f32(mu, (h, w, 4))), _p(_f32(S, (h, w, 4))), _p(c), int(bool(from_variance)), _p(e))
    return e


def next_count(n, max_spp):
    return int(lib().hk_adaptive_next_count(int(n), int(max_spp)))


def converged(e, threshold):
    return bool(lib().hk_adaptive_converged(float(e), float(threshold)))


def groups(ids, counts):
    """adaptive_groups: [(count, [tiles...]), ...] ascending counts, each group in the order of ids"""
    ids = np.ascontiguousarray(ids, np.int32)
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    out_n = np.zeros(max(1, ids.size), np.int32)
    out_len = np.zeros(max(1, ids.size), np.int32)
    out_t = np.zeros(max(1, ids.size), np.int32)
    k = lib().hk_adaptive_groups(_p(ids), int(ids.size), _p(counts), int(counts.size), _p(out_n), _p(out_len), _p(out_t))
    res, off = [], 0
    for g in range(k):
        res.append((int(out_n[g]), [int(t) for t in out_t[off:off + out_len[g]]]))
        off += int(out_len[g])
    return res


def replay(err_at, start, set_ids, min_spp, max_spp, threshold):
    """The schedule of RendererHIP::render_adaptive replayed on the host: err_at(tile, n) -> e_t of `tile` at n samples (float32), start = the
    counts before the call (flat, by raster tile id).  Returns (counts after, rounds, [groups of every round])."""
    n = np.array(start, np.int64).reshape(-1).copy()
    for t in set_ids:
        if n[t] < min_spp:
            n[t] = min_spp
    live = [t for t in set_ids if n[t] < max_spp]
    rounds, history = 0, []
    while live:
        rounds += 1
        go = [t for t in live if not converged(err_at(t, int(n[t])), threshold)]
        history.append(groups(go, n.astype(np.int32)))
        for t in go:
            n[t] = next_count(int(n[t]), max_spp)
        live = [t for t in go if n[t] < max_spp]
    return n.astype(np.int32), rounds, history


def denoise(color, var, feat, n_px, iterations=5, sigma=(4.0, 0.5, 0.1, 0.25, 0.2)):
    """The host build of the denoiser on a ragged frame: color / var [H][W][4] (var as vr_variance gives it), feat [H][W][8], n_px [H][W]"""
    h, w = color.shape[:2]
    n = np.ascontiguousarray(n_px, np.int32)
    assert n.shape == (h, w)
    s = np.asarray(sigma, np.float32)
    out = np.zeros((h, w, 4), np.float32)
    lib().hk_adaptive_denoise(w, h, _p(n), _p(_f32(color, (h, w, 4))), _p(_f32(var, (h, w, 4))), _p(_f32(feat, (h, w, 8))), int(iterations), _p(s), _p(out))
    return out


def prepare(var, feat, n_px):
    h, w = var.shape[:2]
    v = np.zeros((h, w), np.float32)
    g = np.zeros((h, w, 8), np.float32)
    lib().hk_adaptive_denoise_prepare(w, h, _p(np.ascontiguousarray(n_px, np.int32)), _p(_f32(var, (h, w, 4))), _p(_f32(feat, (h, w, 8))), _p(v), _p(g))
    return v, g


# ---- float64 statement of the error estimate (vr_adaptive.h's header comment), written from the formulas, not from the C++ ----------------------
def spec_pixel_error(mu, S, n):
    mu = np.asarray(mu, np.float64)
    S = np.asarray(S, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), mu.shape[:-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.where((n >= 2)[..., None], S * (n / np.maximum(n - 1, 1))[..., None], 0.0)
        s = sum(LUMA[i] * np.sqrt(np.maximum(var[..., i], 0.0)) for i in range(3))
        v = s * s / np.maximum(n, 1)
        L = mu[..., :3] @ np.array(LUMA)
        e = np.sqrt(v) / (L + FLOOR)
    return np.where(n < 2, np.inf, e)


def spec_tile_error(mu, S, counts):
    h, w = mu.shape[:2]
    ty, tx = tiles_of(w, h)
    c = np.broadcast_to(np.asarray(counts), (ty, tx))
    e = spec_pixel_error(mu, S, per_pixel(c, w, h))
    out = np.full((ty, tx), -np.inf)
    for y in range(ty):
        for x in range(tx):
            blk = e[16 * y:16 * y + 16, 16 * x:16 * x + 16]
            out[y, x] = np.nan if np.isnan(blk).any() else blk.max()
    return out
