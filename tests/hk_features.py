"""ctypes binding of tests/hostkernel/libfeatures_host.so: the denoiser feature pass of the product's lane code (vr_trace.h feature_sample /
feature_pixel) built for the host, plus float64 numpy references.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_binding
import hk_common

_lib = None


def build():
    return hk_common.build(__file__, "features_host.cpp", "libfeatures_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _args(o):
    p = o.params()
    dd = hk_binding.grid_desc(o.density)
    ed = hk_binding.grid_desc(o.emission) if o.emission is not None else None
    env = o.env_tex
    keep = (p, dd, ed, env)
    args = [C.byref(p), C.byref(dd), C.byref(ed) if ed is not None else None,
            o.lut.ctypes.data_as(C.c_void_p) if o.lut is not None else None,
            env.ctypes.data_as(C.c_void_p), env.shape[1], env.shape[0], o.impmap.ctypes.data_as(C.c_void_p), 512]
    return args, keep


def samples(o, spp, raw=False):
    """Per (pixel, sample) of an oracle.binding.OracleRenderer's scene: hit [H][W][spp] (bool; raw: feature_sample's result, 0 miss / 1 hit /
    2 lost), values [H][W][spp][7] = t, albedo.rgb, normal.xyz."""
    args, keep = _args(o)
    hit = np.zeros((o.h, o.w, spp), np.int32)
    val = np.zeros((o.h, o.w, spp, 7), np.float32)
    lib().hk_feature_sample(*args, int(spp), hit.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p))
    del keep
    return (hit if raw else hit == 1), val


def feature_pass(o, spp, with_lost=False):
    """The per-pixel pass: [H][W][8] = albedo.rgb, coverage, normal.xyz, depth (with_lost: and the number of pixels that lost a sample)."""
    args, keep = _args(o)
    out = np.zeros((o.h, o.w, 8), np.float32)
    lost = lib().hk_feature_pass(*args, int(spp), out.ctypes.data_as(C.c_void_p))
    del keep
    return (out, lost) if with_lost else out


def aggregate(hit, val):
    """float32 sums in sample order over the per-sample values, divided by the hit count (the per-pixel pass restated in numpy)."""
    h, w, spp = hit.shape
    out = np.zeros((h, w, 8), np.float32)
    for y in range(h):
        for x in range(w):
            n = 0
            s = np.zeros(7, np.float32)
            for k in range(spp):
                if hit[y, x, k]:
                    n += 1
                    s = (s + val[y, x, k]).astype(np.float32)
            if n:
                f = np.float32(n)
                out[y, x, 0:3] = s[1:4] / f
                out[y, x, 3] = f / np.float32(spp)
                out[y, x, 4:7] = s[4:7] / f
                out[y, x, 7] = s[0] / f
    return out


def decoded_grid(g):
    """The density the trilinear filter reads, [z][y][x] float64 (bricks decoded; dense fp16 voxels as they are)."""
    if getattr(g, "dense", None) is not None:
        d = np.asarray(g.dense)
        d = d.view(np.float16) if d.dtype == np.uint16 else d
        ex = g.index_extent
        return d.astype(np.float64).reshape(ex[2], ex[1], ex[0])
    return g.decode_dense().astype(np.float64)


def trilinear(grid, p):
    """common.glsl:289-297 in float64 for points p [N][3] (index space, voxel centres at +0.5, 0 outside the grid)."""
    q = np.asarray(p, np.float64) - 0.5
    i0 = np.floor(q).astype(np.int64)
    f = q - i0
    nz, ny, nx = grid.shape
    out = np.zeros(len(q))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ix, iy, iz = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                ok = (ix >= 0) & (iy >= 0) & (iz >= 0) & (ix < nx) & (iy < ny) & (iz < nz)
                v = np.zeros(len(q))
                v[ok] = grid[iz[ok], iy[ok], ix[ok]]
                w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                out += w * v
    return out


def normals_f64(grid, minv_colmajor, ip):
    """-normalize(transpose(Minv3) g) with g the central difference (one voxel each way) of the float64 trilinear density; also |g|."""
    ip = np.asarray(ip, np.float64)
    g = np.zeros_like(ip)
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        g[:, a] = trilinear(grid, ip + e) - trilinear(grid, ip - e)
    M = np.asarray(minv_colmajor, np.float64).reshape(4, 4).T[:3, :3]
    n = g @ M                                     # row i of the result: transpose(M) @ g_i
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return -n / np.where(ln > 0, ln, 1.0), np.linalg.norm(g, axis=1)
