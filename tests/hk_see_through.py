"""ctypes binding of tests/hostkernel/libsee_through_host.so: the see-through tile classifier (vr_sky_tiles.h) and the sample of such a tile (vr_trace.h
sky_sample without its box test) of the product built for the host, plus an independent float64 numpy statement of "can a camera ray of this tile come within
tap reach of a live brick": a lattice of slab tests in index space against every live brick grown by 2.5 voxels.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_binding
import hk_common
from hk_common import _p

_lib = None
MARCH, CLEAR, SEE = 0, 1, 2
STEP = 4            # lattice points per pixel and axis
REACH = 2.5         # voxels a tap reaches beyond its point (tricubic_tap_t: floor(p - 0.5) - 1 ... + 2)


def build():
    return hk_common.build(__file__, "see_through_host.cpp", "libsee_through_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_st_uniforms_size.restype = C.c_int
        L.hk_st_classify.restype = C.c_longlong
        L.hk_st_live.restype = C.c_int
        L.hk_st_cell_grow.restype = C.c_double
        L.hk_st_tap_reach.restype = C.c_double
        _lib = L
    return _lib


def tiles_of(w, h):
    return (w + 15) // 16, (h + 15) // 16


def _params(orc, **override):
    p = orc.params()
    assert C.sizeof(p) == lib().hk_st_uniforms_size(), (C.sizeof(p), lib().hk_st_uniforms_size())
    for k, v in override.items():
        setattr(p, k, v)
    return p


def _table(orc, rng, held):
    """(range words or None, nb) as the renderer would hand them over: None = a grid whose table the host does not hold"""
    g = orc.density
    nb = np.array(g.n_bricks, np.int32)
    words = np.ascontiguousarray(g.range if rng is None else rng, np.uint32)
    assert words.size == int(nb.prod())
    return (words if held else None), nb


def classify(orc, tiles=None, rng=None, held=True, **override):
    """(cls[i] in {MARCH, CLEAR, SEE} for tile ids `tiles` (default: every tile of the frame), pyramid cells visited or -1 for the fallback).
    rng: other range words than the grid's own; override: fields of the uniform block set after the oracle filled it"""
    nx, ny = tiles_of(orc.w, orc.h)
    t = np.ascontiguousarray(np.arange(nx * ny) if tiles is None else tiles, np.int32)
    out = np.zeros(t.size, np.uint8)
    p = _params(orc, **override)
    words, nb = _table(orc, rng, held)
    visited = lib().hk_st_classify(C.byref(p), _p(words) if words is not None else None, _p(nb), _p(t), int(t.size), _p(out))
    return out, int(visited)


def split(orc, ids=()):
    """(march, clear, see-through) lists of sky_split_tiles3; ids empty = the whole frame"""
    nx, ny = tiles_of(orc.w, orc.h)
    ids = np.ascontiguousarray(ids, np.int32)
    n = ids.size if ids.size else nx * ny
    out = np.zeros(n, np.int32)
    counts = np.zeros(3, np.int32)
    p = _params(orc)
    words, nb = _table(orc, None, True)
    lib().hk_st_split(C.byref(p), _p(words), _p(nb), _p(ids), int(ids.size), nx * ny, _p(out), _p(counts))
    a, b = int(counts[0]), int(counts[0] + counts[1])
    return out[:a], out[a:b], out[b:]


def samples(orc, items):
    """sky_sample without the box test of [n][3] (px, py, sample number): [n][4] float32"""
    items = np.ascontiguousarray(items, np.int32)
    n = items.shape[0]
    out = np.zeros((n, 4), np.float32)
    p = _params(orc)
    dd = hk_binding.grid_desc(orc.density)
    env = orc.env_tex
    lib().hk_st_samples(C.byref(p), C.byref(dd), _p(env), env.shape[1], env.shape[0], _p(orc.impmap), 512, _p(items), n, _p(out))
    return out


# ---- the independent statement ----------------------------------------------------------------------------------------------------------------------
def live_bricks(orc, rng=None):
    """[n][3] brick coordinates (x, y, z) of the live bricks: not (min <= 0 and max <= 0), a NaN half counts as live"""
    g = orc.density
    nbx, nby, nbz = g.n_bricks
    w = np.ascontiguousarray(g.range if rng is None else rng, np.uint32)
    lo = (w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    hi = (w >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):
        live = ~((lo <= 0) & (hi <= 0))
    z, y, x = np.nonzero(live.reshape(nbz, nby, nbx))
    return np.stack([x, y, z], 1).astype(np.float64)


def tile_rect(t, w, h):
    nx, _ = tiles_of(w, h)
    x0, y0 = (t % nx) * 16, (t // nx) * 16
    return x0, y0, min(x0 + 16, w), min(y0 + 16, h)


def lattice_touches(orc, tiles, grow=REACH, rng=None, cull=True):
    """touch[i]: some ray of the quarter-pixel lattice over the closed pixel rectangle of tile tiles[i] -- edges included -- passes the slab test in double
    (t_near <= t_far, t >= 0) against a live brick's box [8 b - grow, 8 b + 8 + grow] in index space.  The ray is do_new's, cam_transform (column-major)
    * ((x - W/2) / H, (y - H/2) / H, cam_z), taken to index space by the inverse of vol_density_transform formed here in double."""
    p = orc.params()
    W, H = orc.w, orc.h
    M = np.array(p.cam_transform[:], np.float64).reshape(3, 3).T
    cam = np.array(p.cam_pos[:], np.float64)
    cam_z = -0.5 / np.tan(0.5 * np.pi * float(np.float32(p.cam_fov)) / 180.0)
    T = np.linalg.inv(np.array(p.vol_density_transform[:], np.float64).reshape(4, 4).T)      # world -> index
    o = T[:3, :3] @ cam + T[:3, 3]
    b = live_bricks(orc, rng)
    lo, hi = 8.0 * b - grow, 8.0 * b + 8.0 + grow
    out = np.zeros(len(tiles), bool)
    for i, t in enumerate(tiles):
        x0, y0, x1, y1 = tile_rect(int(t), W, H)
        x = np.arange((x1 - x0) * STEP + 1, dtype=np.float64) / STEP + x0
        y = np.arange((y1 - y0) * STEP + 1, dtype=np.float64) / STEP + y0
        X, Y = np.meshgrid(x, y)
        d = np.stack([(X.ravel() - 0.5 * W) / H, (Y.ravel() - 0.5 * H) / H, np.full(X.size, cam_z)], 1) @ M.T
        d = d @ T[:3, :3].T
        # Only the bricks the tile's rays can come near take the slab tests.  The rays of a rectangle are the positive combinations of its four corner rays, so they
        # lie in the cone around the centre ray that holds the corners; a grown brick lies in the sphere around its centre that holds its box.  A ray of the cone
        # can meet the sphere only if the sphere's centre is within (cone angle + the sphere's angular radius) of the axis -- or the origin is in the sphere.
        unit = d / np.linalg.norm(d, axis=1, keepdims=True)
        axis_ = unit[(len(y) // 2) * len(x) + len(x) // 2]
        cone = np.arccos(np.clip(unit[[0, len(x) - 1, -len(x), -1]] @ axis_, -1.0, 1.0)).max()
        cb, rad = 8.0 * b + 4.0 - o, np.sqrt(3.0) * (4.0 + grow)
        dist = np.linalg.norm(cb, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            off = np.arccos(np.clip((cb @ axis_) / dist, -1.0, 1.0))
            near = (dist <= rad) | (off <= cone + np.arcsin(np.clip(rad / dist, 0.0, 1.0)) + 1e-9)
        if not cull:                  # (the tests check once that the cull changes no answer)
            near[:] = True
        tlo, thi = lo[near], hi[near]
        for r0 in range(0, d.shape[0], 128):
            if not len(tlo):
                break
            dd = d[r0:r0 + 128, None, :]
            with np.errstate(divide="ignore", invalid="ignore"):
                t0, t1 = (tlo[None] - o) / dd, (thi[None] - o) / dd
            tn = np.fmax(np.fmin(t0, t1).max(2), 0.0)
            tf = np.fmax(t0, t1).min(2)
            if (tn <= tf).any():
                out[i] = True
                break
    return out
