"""ctypes binding of tests/hostkernel/libsky_host.so: the clear-tile classifier (vr_sky_tiles.h) and the primary-miss sample (vr_trace.h sky_sample) of the
product built for the host, plus an independent float64 numpy statement of "can a camera ray of this tile hit the box": a lattice of slab tests.
TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_binding
import hk_common
from hk_common import _p

_lib = None


def build():
    return hk_common.build(__file__, "sky_host.cpp", "libsky_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_sky_uniforms_size.restype = C.c_int
        L.hk_sky_split.restype = C.c_int
        _lib = L
    return _lib


def tiles_of(w, h):
    return (w + 15) // 16, (h + 15) // 16


def _params(orc):
    p = orc.params()
    assert C.sizeof(p) == lib().hk_sky_uniforms_size(), (C.sizeof(p), lib().hk_sky_uniforms_size())
    return p


def classify(orc, tiles=None):
    """clear[i] for tile ids `tiles` (default: every tile of the frame) of the view held by an oracle.binding.OracleRenderer"""
    nx, ny = tiles_of(orc.w, orc.h)
    t = np.ascontiguousarray(np.arange(nx * ny) if tiles is None else tiles, np.int32)
    out = np.zeros(t.size, np.uint8)
    p = _params(orc)
    lib().hk_sky_classify(C.byref(p), _p(t), int(t.size), _p(out))
    return out.astype(bool)


def split(orc, ids=()):
    """(march list, clear list) of sky_split_tiles; ids empty = the whole frame"""
    nx, ny = tiles_of(orc.w, orc.h)
    ids = np.ascontiguousarray(ids, np.int32)
    n = ids.size if ids.size else nx * ny
    out = np.zeros(n, np.int32)
    p = _params(orc)
    k = lib().hk_sky_split(C.byref(p), _p(ids), int(ids.size), nx * ny, _p(out))
    return out[:n - k], out[n - k:]


def samples(orc, items):
    """sky_sample of [n][3] (px, py, sample number): ([n][4] float32, [n] bool missed)"""
    items = np.ascontiguousarray(items, np.int32)
    n = items.shape[0]
    out = np.zeros((n, 4), np.float32)
    miss = np.zeros(n, np.int32)
    p = _params(orc)
    dd = hk_binding.grid_desc(orc.density)
    env, lut = orc.env_tex, orc.lut
    lib().hk_sky_samples(C.byref(p), C.byref(dd), _p(lut) if lut is not None else None, _p(env), env.shape[1], env.shape[0], _p(orc.impmap), 512,
                         _p(items), n, _p(out), _p(miss))
    return out, miss.astype(bool)


# ---- the independent statement ----------------------------------------------------------------------------------------------------------------------
MARGIN = 2          # pixels the lattice extends beyond the frame on every side
STEP = 4            # lattice points per pixel and axis


def lattice_hits(orc):
    """hit[j][i]: the ray through image-plane point (x, y) = (i / STEP - MARGIN, j / STEP - MARGIN) in continuous pixel coordinates -- pixel px covers
    [px, px + 1] -- meets the volume's box, by the slab test in double, edges included (t_near <= t_far, t_near >= 0).  The ray is do_new's:
    cam_transform (column-major) * ((x - W/2) / H, (y - H/2) / H, cam_z), cam_z = -0.5 / tan(fov / 2)."""
    p = orc.params()
    W, H = orc.w, orc.h
    M = np.array(p.cam_transform[:], np.float64).reshape(3, 3).T        # M[r][c] = m[3 c + r]
    cam = np.array(p.cam_pos[:], np.float64)
    lo, hi = np.array(p.vol_bb_min[:], np.float64), np.array(p.vol_bb_max[:], np.float64)
    cam_z = -0.5 / np.tan(0.5 * np.pi * float(np.float32(p.cam_fov)) / 180.0)
    x = np.arange((W + 2 * MARGIN) * STEP + 1, dtype=np.float64) / STEP - MARGIN
    y = np.arange((H + 2 * MARGIN) * STEP + 1, dtype=np.float64) / STEP - MARGIN
    fx, fy = (x - 0.5 * W) / H, (y - 0.5 * H) / H
    tnear = np.zeros((y.size, x.size))
    tfar = np.full((y.size, x.size), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            d = M[a, 0] * fx[None, :] + M[a, 1] * fy[:, None] + M[a, 2] * cam_z
            t0, t1 = (lo[a] - cam[a]) / d, (hi[a] - cam[a]) / d
            tnear = np.fmax(tnear, np.fmin(t0, t1))
            tfar = np.fmin(tfar, np.fmax(t0, t1))
    return tnear <= tfar


def lattice_clear(hits, w, h, margin):
    """clear[t] for every raster tile: no lattice point of its closed pixel rectangle (inside the frame), grown by `margin` pixels, hits"""
    assert 0 <= margin <= MARGIN
    nx, ny = tiles_of(w, h)
    out = np.zeros(nx * ny, bool)
    for t in range(nx * ny):
        x0, y0 = (t % nx) * 16, (t // nx) * 16
        x1, y1 = min(x0 + 16, w), min(y0 + 16, h)
        i0, i1 = (x0 - margin + MARGIN) * STEP, (x1 + margin + MARGIN) * STEP
        j0, j1 = (y0 - margin + MARGIN) * STEP, (y1 + margin + MARGIN) * STEP
        out[t] = not hits[j0:j1 + 1, i0:i1 + 1].any()
    return out
