"""ctypes binding of tests/hostkernel/libexpected_host.so: the expected-value feature pass (volren_amd/csrc/vr_expected.h expected_pixel) built for the
host, plus a float64 numpy statement of the same definition, written from the header's text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_features

_lib = None
MAX_STEPS = 4096
MIN_T = 2.0 ** -10


def build():
    return hk_common.build(__file__, "expected_host.cpp", "libexpected_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def expected_pass(o, rays, with_info=False):
    """The per-pixel pass on an oracle.binding.OracleRenderer's scene: [H][W][8] float32 = albedo.rgb, coverage, normal.xyz, depth.
    with_info: and per sub-ray (j * rays + i) m [H][W][rays^2] (0: contributed nothing), the steps it ran, the transmittance it ended with."""
    args, keep = hk_features._args(o)
    out = np.zeros((o.h, o.w, 8), np.float32)
    info = np.zeros((o.h, o.w, rays * rays, 3), np.int32) if with_info else None
    lib().hk_expected_pass(*args, int(rays), out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p) if with_info else None)
    del keep
    if not with_info:
        return out
    return out, info[..., 0].copy(), info[..., 1].copy(), np.ascontiguousarray(info[..., 2]).view(np.float32)


# ---- the float64 statement -----------------------------------------------------------------------------------------------------------------------
def corners(grid, p):
    """the eight corner values [N][8] in [z][y][x] order (0 outside the grid) and the weights f [N][3] of the trilinear filter at index-space points p"""
    q = np.asarray(p, np.float64) - 0.5
    fl = np.floor(q)
    f = q - fl
    i0 = fl.astype(np.int64)
    nz, ny, nx = grid.shape
    v = np.zeros((len(q), 8))
    for c in range(8):
        ix, iy, iz = i0[:, 0] + (c & 1), i0[:, 1] + ((c >> 1) & 1), i0[:, 2] + (c >> 2)
        ok = (ix >= 0) & (iy >= 0) & (iz >= 0) & (ix < nx) & (iy < ny) & (iz < nz)
        v[ok, c] = grid[iz[ok], iy[ok], ix[ok]]
    return v, f


def _mix(x, y, a):
    return x * (1.0 - a) + y * a


def value_and_gradient(v, f):
    """the trilinear interpolant of corners v at weights f, and its gradient in voxel units"""
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    val = _mix(_mix(_mix(v[:, 0], v[:, 1], fx), _mix(v[:, 2], v[:, 3], fx), fy), _mix(_mix(v[:, 4], v[:, 5], fx), _mix(v[:, 6], v[:, 7], fx), fy), fz)
    gx = _mix(_mix(v[:, 1] - v[:, 0], v[:, 3] - v[:, 2], fy), _mix(v[:, 5] - v[:, 4], v[:, 7] - v[:, 6], fy), fz)
    gy = _mix(_mix(v[:, 2] - v[:, 0], v[:, 3] - v[:, 1], fx), _mix(v[:, 6] - v[:, 4], v[:, 7] - v[:, 5], fx), fz)
    gz = _mix(_mix(v[:, 4] - v[:, 0], v[:, 5] - v[:, 1], fx), _mix(v[:, 6] - v[:, 2], v[:, 7] - v[:, 3], fx), fy)
    return val, np.stack([gx, gy, gz], 1)


def tf_lookup(p, lut, d):
    """common.glsl:203-212 in float64: [N][4]"""
    n = int(p.tf_size)
    tc = np.clip((d - float(p.tf_window_left)) / float(p.tf_window_width), 0.0, float(np.float32(1.0) - np.float32(1e-6)))
    tcs = tc * n
    idx = np.clip(np.floor(tcs).astype(np.int64), 0, n - 1)
    f = tcs - np.floor(tcs)
    idx1 = np.minimum(idx + 1, n - 1)
    lut = np.asarray(lut, np.float64).reshape(n, 4)
    return lut[idx] * (1.0 - f[:, None]) + lut[idx1] * f[:, None]


def spec_expected(o, rays):
    """vr_expected.h's header comment in float64, all sub-rays of the frame side by side.  -> out [H][W][8] float64, m [H][W][rays^2], steps run"""
    p = o.params()
    W, H, n = o.w, o.h, int(rays)
    grid = hk_features.decoded_grid(o.density)
    lut = None if o.lut is None else np.asarray(o.lut, np.float64)
    cam_z = -0.5 / np.tan(0.5 * np.pi * float(p.cam_fov) / 180.0)
    y, x, j, i = np.meshgrid(np.arange(H), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    x, y, i, j = (a.reshape(-1).astype(np.float64) for a in (x, y, i, j))
    N = len(x)
    fx = ((x + (i + 0.5) / n) - W * 0.5) / H
    fy = ((y + (j + 0.5) / n) - H * 0.5) / H
    d = np.stack([fx, fy, np.full(N, cam_z)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ct = np.array(list(p.cam_transform), np.float64).reshape(3, 3).T                 # column-major
    d = d @ ct.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = np.array(list(p.cam_pos), np.float64)
    bmin, bmax = np.array(list(p.vol_bb_min), np.float64), np.array(list(p.vol_bb_max), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        lo, hi = (bmin - pos) * inv, (bmax - pos) * inv
        tnear = np.maximum(0.0, np.minimum(lo, hi).max(axis=1))
        tfar = np.maximum(lo, hi).min(axis=1)
    M = np.array(list(p.vol_density_inv_transform), np.float64).reshape(4, 4).T
    ipos = M[:3, :3] @ pos + M[:3, 3]
    idir = d @ M[:3, :3].T
    L = np.linalg.norm(idir, axis=1)
    with np.errstate(invalid="ignore"):
        live = (tnear <= tfar) & (tfar > tnear) & np.isfinite(L) & np.isfinite(tnear) & np.isfinite(tfar)
    length = np.where(live, tfar - tnear, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(live, np.clip(np.ceil(length * L), 1, MAX_STEPS), 0).astype(np.int64)
    h = length / np.maximum(m, 1)
    scale, alb = float(p.vol_density_scale), np.array(list(p.vol_albedo), np.float64)
    T = np.ones(N)
    K, D, A, Nn = np.zeros(N), np.zeros(N), np.zeros((N, 3)), np.zeros((N, 3))
    steps = np.zeros(N, np.int64)
    running = live.copy()
    for k in range(int(m.max()) if N else 0):
        running &= k < m
        r = np.flatnonzero(running)
        if not len(r):
            break
        steps[r] += 1
        t = tnear[r] + (k + 0.5) * h[r]
        v, f = corners(grid, ipos[None, :] + t[:, None] * idir[r])
        raw, g = value_and_gradient(v, f)
        sigma = scale * raw
        a = np.broadcast_to(alb, (len(r), 3))
        if lut is not None:
            rgba = tf_lookup(p, lut, sigma * float(p.vol_inv_majorant))
            sigma = rgba[:, 3] * float(p.vol_majorant)
            a = alb[None, :] * rgba[:, :3]
        on = sigma > 0
        e = np.exp(-(sigma * h[r]))
        w = np.where(on, T[r] * (1.0 - e), 0.0)
        nn = g @ M[:3, :3]                                                            # row i: transpose(Minv3) g_i
        ln = np.linalg.norm(nn, axis=1, keepdims=True)
        nh = -nn / np.where(ln > 0, ln, 1.0)
        K[r] += w
        D[r] += w * t
        A[r] += w[:, None] * a
        Nn[r] += w[:, None] * nh
        T[r] = np.where(on, T[r] * e, T[r])
        running[r[on & (T[r] <= MIN_T)]] = False
    shape = (H, W, n * n)
    Kp, Dp = K.reshape(shape).sum(axis=2), D.reshape(shape).sum(axis=2)
    Ap, Np = A.reshape(shape + (3,)).sum(axis=2), Nn.reshape(shape + (3,)).sum(axis=2)
    out = np.zeros((H, W, 8))
    hit = Kp > 0
    Ks = np.where(hit, Kp, 1.0)
    out[..., 0:3] = Ap / Ks[..., None]
    out[..., 3] = Kp / (n * n)
    out[..., 4:7] = Np / Ks[..., None]
    out[..., 7] = Dp / Ks
    out[~hit] = 0.0
    return out, m.reshape(shape), steps.reshape(shape)
