"""ctypes binding of tests/hostkernel/libexpected_skip_host.so: the clear-distance table (volren_amd/csrc/vr_clear.h) and the expected-value march that
skips empty space by it (vr_expected.h) built for the host, plus numpy statements of the table's definition and of the work the march has left,
written from the headers' text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_features

_lib = None
WORK = ("rays", "steps", "fetched", "reads", "audit")


def build():
    return hk_common.build(__file__, "expected_skip_host.cpp", "libexpected_skip_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def table(o):
    """the host-built clear-distance table of an oracle.binding.OracleRenderer's density grid: uint8 [cz][cy][cx]"""
    args, keep = hk_features._args(o)
    n = (C.c_int32 * 3)()
    lib().hk_clear_table(*args, None, n)
    out = np.zeros((n[2], n[1], n[0]), np.uint8)
    lib().hk_clear_table(*args, out.ctypes.data_as(C.c_void_p), n)
    del keep
    return out


def expected_pass(o, rays, skip):
    """hk_expected.expected_pass(o, rays, with_info=True) with the table: skip 0 marches every step, 1 skips, 2 skips and audits.
    -> out [H][W][8], m, steps [H][W][rays^2], T, work {rays, steps, fetched, reads, audit}"""
    args, keep = hk_features._args(o)
    out = np.zeros((o.h, o.w, 8), np.float32)
    info = np.zeros((o.h, o.w, rays * rays, 3), np.int32)
    work = np.zeros(5, np.uint64)
    lib().hk_expected_skip_pass(*args, int(rays), int(skip), out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p), work.ctypes.data_as(C.c_void_p))
    del keep
    return out, info[..., 0].copy(), info[..., 1].copy(), np.ascontiguousarray(info[..., 2]).view(np.float32), dict(zip(WORK, (int(v) for v in work)))


# ---- the numpy statements ------------------------------------------------------------------------------------------------------------------------
def decoded_bits(g):
    """the bit patterns of the voxels as the taps decode them in float32, uint32 [z][y][x]: rmin + unorm8 * rdiff for bricks (oracle.binding.Grid.decode_dense
    evaluates exactly that in float32), the fp16 voxel for dense grids"""
    if getattr(g, "dense", None) is not None:
        d = np.asarray(g.dense)
        d = d.view(np.float16) if d.dtype == np.uint16 else d
        ex = g.index_extent
        return np.ascontiguousarray(d.astype(np.float32).reshape(ex[2], ex[1], ex[0])).view(np.uint32)
    return np.ascontiguousarray(g.decode_dense(), np.float32).view(np.uint32)


def _windows(a, axis, n, width, stride):
    """OR over the `width` slices of `a` along `axis` that start at stride * c, c < n"""
    out = None
    for d in range(width):
        s = np.take(a, np.arange(d, d + stride * n, stride), axis=axis)
        out = s if out is None else out | s
    return out


def spec_table(g):
    """vr_clear.h's text: a cell of 8^3 voxels is clear when every voxel of its box grown by one voxel is +0 as a bit pattern (voxels outside the grid are);
    the byte is min(255, Chebyshev distance in cells to the nearest cell that is not clear).  By dilation, one cell at a time."""
    bits = decoded_bits(g)
    nz, ny, nx = bits.shape
    n = [(v + 7) // 8 for v in (nz, ny, nx)]
    live = np.zeros((8 * n[0] + 2, 8 * n[1] + 2, 8 * n[2] + 2), bool)
    live[1:1 + nz, 1:1 + ny, 1:1 + nx] = bits != 0
    for axis in range(3):
        live = _windows(live, axis, n[axis], 10, 8)
    out = np.where(live, 0, 255).astype(np.uint8)
    reach = live.copy()
    for r in range(1, 255):
        grown = reach
        for axis in range(3):
            p = np.pad(grown, [(1, 1) if a == axis else (0, 0) for a in range(3)])
            grown = _windows(p, axis, grown.shape[axis], 3, 1)
        new = grown & ~reach
        if not new.any():
            break
        out[new] = r
        reach = grown
    return out


def spec_fetched(o, tab, steps, rays=1):
    """The steps that still fetch their corners, by the headers' rule in float64: of the steps k < steps[sub-ray] (the step index the march reached), those whose
    midpoint lies outside the table or in a cell with byte 0.  tab: the table [cz][cy][cx]; steps: [H][W][rays^2]."""
    p = o.params()
    W, H, n = o.w, o.h, int(rays)
    cam_z = -0.5 / np.tan(0.5 * np.pi * float(p.cam_fov) / 180.0)
    y, x, j, i = np.meshgrid(np.arange(H), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    x, y, i, j = (a.reshape(-1).astype(np.float64) for a in (x, y, i, j))
    d = np.stack([((x + (i + 0.5) / n) - W * 0.5) / H, ((y + (j + 0.5) / n) - H * 0.5) / H, np.full(len(x), cam_z)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ np.array(list(p.cam_transform), np.float64).reshape(3, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = np.array(list(p.cam_pos), np.float64)
    bmin, bmax = np.array(list(p.vol_bb_min), np.float64), np.array(list(p.vol_bb_max), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo, hi = (bmin - pos) / d, (bmax - pos) / d
        tnear = np.maximum(0.0, np.minimum(lo, hi).max(axis=1))
        tfar = np.maximum(lo, hi).min(axis=1)
    M = np.array(list(p.vol_density_inv_transform), np.float64).reshape(4, 4).T
    ipos, idir = M[:3, :3] @ pos + M[:3, 3], d @ M[:3, :3].T
    steps = np.asarray(steps).reshape(-1)
    live = steps > 0
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(live, np.clip(np.ceil((tfar - tnear) * np.linalg.norm(idir, axis=1)), 1, 4096), 1)
    h = np.where(live, tfar - tnear, 0.0) / m
    nz, ny, nx = tab.shape
    fetched = 0
    for k in range(int(steps.max())):
        r = np.flatnonzero(steps > k)
        ip = ipos[None, :] + (tnear[r] + (k + 0.5) * h[r])[:, None] * idir[r]
        c = np.floor(ip / 8.0).astype(np.int64)
        inside = (c >= 0).all(axis=1) & (c[:, 0] < nx) & (c[:, 1] < ny) & (c[:, 2] < nz)
        byte = np.zeros(len(r), np.int64)
        byte[inside] = tab[c[inside, 2], c[inside, 1], c[inside, 0]]
        fetched += int((byte == 0).sum())
    return fetched
