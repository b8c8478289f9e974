"""ctypes binding of tests/hostkernel/libexpected_cubic_host.so: the cubic B-spline lookup (volren_amd/csrc/vr_cubic.h), the clear-distance table of
either reach (vr_clear.h) and the expected-value march on either field (vr_expected.h, CUBIC) built for the host, plus float64 / numpy statements of
the same definitions, written from the headers' text.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
import hk_expected as he
import hk_expected_skip as hs
import hk_features

_lib = None
WORK = hs.WORK


def build():
    return hk_common.build(__file__, "expected_cubic_host.cpp", "libexpected_cubic_host.so", ("-Wno-unknown-pragmas", "-Wno-subobject-linkage", "-DVR_HOST_TRACE"))


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.hc_violations.restype = C.c_longlong
        _lib.hc_taps.restype = C.c_longlong
    return _lib


def violations():
    """(taps that fell outside their table, taps checked) since the last reset()"""
    return int(lib().hc_violations()), int(lib().hc_taps())


def reset():
    lib().hc_reset()


def words(points):
    """index-space points [n][3] as the uint32 bit patterns of their float32 values (uint32 input is taken as bits already)"""
    p = np.asarray(points)
    return np.ascontiguousarray(p if p.dtype == np.uint32 else p.astype(np.float32).view(np.uint32)).reshape(-1, 3)


def brick_arrays(vox):
    """The arrays of a brick grid of integer voxel values 0..255 [z][y][x] (extents multiples of 8), every brick with the range (0, 255) -- a voxel decodes to
    its integer exactly -- and its own block of the atlas, in the layout of encoder_ref.encode_arrays."""
    import scenes
    vox = np.ascontiguousarray(vox, np.uint8)
    nz, ny, nx = (v // 8 for v in vox.shape)
    n = nx * ny * nz
    ind = np.array([(bx << 22) | (by << 12) | (bz << 2) for bz in range(nz) for by in range(ny) for bx in range(nx)], np.uint32)
    rng = np.full(n, int(np.array(255.0, np.float16).view(np.uint16)) << 16, np.uint32)
    mips = scenes._range_mips(np.zeros((nz, ny, nx), np.float32), np.full((nz, ny, nx), 255.0, np.float32))
    return dict(transform=np.eye(4, dtype=np.float32).reshape(16), n_bricks=(nx, ny, nz), min_maj=(0.0, 255.0), brick_counter=n, indirection=ind, rng=rng,
                atlas_dim=(8 * nx, 8 * ny, 8 * nz), atlas=vox.reshape(-1), mips=mips)


def oracle_brick_grid(a):
    from oracle import binding as ob
    g = ob.Grid()
    g.set(a["transform"], a["n_bricks"], a["min_maj"], a["brick_counter"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"])
    return g


def catalogue(extent):
    """The point catalogue of the lookup's tests for a grid of extent (x, y, z) voxels, float32 [n][3].  Per axis: voxel centres (t = 0) and the float below
    each (t = the float below 1); the brick face at 8 from both sides; every quarter voxel within two and a half voxels of each border, inside and beyond it;
    negative coordinates (floor, not truncation); -0 and a denormal.  All triples of those; then NaN, +-inf and +-2^30 on one axis at a time."""
    axes = []
    for n in extent:
        c = np.arange(0, n, dtype=np.float32) + np.float32(0.5)
        v = [c, np.nextafter(c, np.float32(-np.inf)), np.arange(-10, 11, dtype=np.float32) * np.float32(0.25), np.float32(n) + np.arange(-10, 11, dtype=np.float32) * np.float32(0.25),
             np.array([-3.2, -1.75, -0.3, -0.0, 1e-40], np.float32)]
        if n > 8:
            v.append(np.array([np.nextafter(np.float32(8), np.float32(0)), 8.0, np.nextafter(np.float32(8), np.float32(9)), 7.5, 8.5], np.float32))
        axes.append(np.unique(np.concatenate(v).astype(np.float32).view(np.uint32)).view(np.float32))
    X, Y, Z = np.meshgrid(axes[0], axes[1], axes[2], indexing="ij")
    pts = [np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], 1)]
    mid = np.array([0.4 * n + 0.3 for n in extent], np.float32)
    for a in range(3):
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 30, -2.0 ** 30):
            for other in (mid, np.array([-0.0, 1e-40, 0.5], np.float32)):
                q = other.copy()
                q[a] = bad
                pts.append(q[None, :])
    return np.concatenate(pts).astype(np.float32)


def probe(o, points):
    """cubic_lookup on the density grid of an oracle.binding.OracleRenderer at points [n][3]: [n][4] float32 = value, gx, gy, gz"""
    args, keep = hk_features._args(o)
    w = words(points)
    out = np.zeros((len(w), 4), np.float32)
    lib().hc_cubic_probe(*args, w.ctypes.data_as(C.c_void_p), C.c_longlong(len(w)), out.ctypes.data_as(C.c_void_p))
    del keep
    return out


def table(o, reach):
    """the host-built clear-distance table of that reach (1 or 2): uint8 [cz][cy][cx]"""
    args, keep = hk_features._args(o)
    n = (C.c_int32 * 3)()
    lib().hc_clear_table(*args, int(reach), None, n)
    out = np.zeros((n[2], n[1], n[0]), np.uint8)
    lib().hc_clear_table(*args, int(reach), out.ctypes.data_as(C.c_void_p), n)
    del keep
    return out


def expected_pass(o, rays, field, skip=0, reach=0):
    """hk_expected_skip.expected_pass with the field: 0 trilinear, 1 the tracker's.  skip 0 marches every step, 1 skips, 2 skips and audits; reach 0: the
    table the field marches with, 1 | 2: that table whatever the field.
    -> out [H][W][8], m, steps [H][W][rays^2], T, work {rays, steps, fetched, reads, audit}"""
    args, keep = hk_features._args(o)
    out = np.zeros((o.h, o.w, 8), np.float32)
    info = np.zeros((o.h, o.w, rays * rays, 3), np.int32)
    work = np.zeros(5, np.uint64)
    lib().hc_expected_pass(*args, int(rays), int(field), int(skip), int(reach), out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p),
                           work.ctypes.data_as(C.c_void_p))
    del keep
    return out, info[..., 0].copy(), info[..., 1].copy(), np.ascontiguousarray(info[..., 2]).view(np.float32), dict(zip(WORK, (int(v) for v in work)))


# ---- the float64 statements ------------------------------------------------------------------------------------------------------------------------
def axis_weights(t):
    """the four B-spline weights and their derivatives at t [N]: [N][4] each"""
    t2, t3 = t * t, t * t * t
    w = np.stack([-t3 + 3 * t2 - 3 * t + 1, 3 * t3 - 6 * t2 + 4, -3 * t3 + 3 * t2 + 3 * t + 1, t3], 1) / 6.0
    d = np.stack([-t2 + 2 * t - 1, 3 * t2 - 4 * t, -3 * t2 + 2 * t + 1, t2], 1) / 2.0
    return w, d


def cubic(grid, p):
    """vr_cubic.h in float64: value [N] and gradient [N][3] (voxel units) of the separable cubic B-spline of grid [z][y][x] at index-space points p [N][3];
    voxels outside the grid are 0"""
    q = np.asarray(p, np.float64) - 0.5
    fl = np.floor(q)
    t = q - fl
    i0 = fl.astype(np.int64) - 1
    nz, ny, nx = grid.shape
    wx, dx = axis_weights(t[:, 0])
    wy, dy = axis_weights(t[:, 1])
    wz, dz = axis_weights(t[:, 2])
    val, g = np.zeros(len(q)), np.zeros((len(q), 3))
    for k in range(4):
        for j in range(4):
            for i in range(4):
                ix, iy, iz = i0[:, 0] + i, i0[:, 1] + j, i0[:, 2] + k
                ok = (ix >= 0) & (iy >= 0) & (iz >= 0) & (ix < nx) & (iy < ny) & (iz < nz)
                v = np.zeros(len(q))
                v[ok] = grid[iz[ok], iy[ok], ix[ok]]
                val += wz[:, k] * wy[:, j] * wx[:, i] * v
                g[:, 0] += wz[:, k] * wy[:, j] * dx[:, i] * v
                g[:, 1] += wz[:, k] * dy[:, j] * wx[:, i] * v
                g[:, 2] += dz[:, k] * wy[:, j] * wx[:, i] * v
    return val, g


def spec_table(g, reach):
    """vr_clear.h's text at that reach: a cell of 8^3 voxels is clear when every voxel of its box grown by `reach` voxels is +0 as a bit pattern (voxels
    outside the grid are); the byte is min(255, Chebyshev distance in cells to the nearest cell that is not clear)"""
    bits = hs.decoded_bits(g)
    nz, ny, nx = bits.shape
    n = [(v + 7) // 8 for v in (nz, ny, nx)]
    live = np.zeros((8 * n[0] + 2 * reach, 8 * n[1] + 2 * reach, 8 * n[2] + 2 * reach), bool)
    live[reach:reach + nz, reach:reach + ny, reach:reach + nx] = bits != 0
    for axis in range(3):
        live = hs._windows(live, axis, n[axis], 8 + 2 * reach, 8)
    out = np.where(live, 0, 255).astype(np.uint8)
    front = live.copy()
    for r in range(1, 255):
        grown = front
        for axis in range(3):
            p = np.pad(grown, [(1, 1) if a == axis else (0, 0) for a in range(3)])
            grown = hs._windows(p, axis, grown.shape[axis], 3, 1)
        new = grown & ~front
        if not new.any():
            break
        out[new] = r
        front = grown
    return out


def spec_expected(o, rays, field):
    """vr_expected.h's header comment in float64 with the Density and Normal lines of `field` (0: hk_expected.spec_expected's trilinear ones; 1: without a
    LUT the cubic B-spline field), all sub-rays of the frame side by side.  -> out [H][W][8] float64, m [H][W][rays^2], steps run"""
    if not field or o.lut is not None:
        return he.spec_expected(o, rays)
    p = o.params()
    W, H, n = o.w, o.h, int(rays)
    grid = hk_features.decoded_grid(o.density)
    cam_z = -0.5 / np.tan(0.5 * np.pi * float(p.cam_fov) / 180.0)
    y, x, j, i = np.meshgrid(np.arange(H), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    x, y, i, j = (a.reshape(-1).astype(np.float64) for a in (x, y, i, j))
    N = len(x)
    d = np.stack([((x + (i + 0.5) / n) - W * 0.5) / H, ((y + (j + 0.5) / n) - H * 0.5) / H, np.full(N, cam_z)], 1)
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
        m = np.where(live, np.clip(np.ceil(length * L), 1, he.MAX_STEPS), 0).astype(np.int64)
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
        raw, g = cubic(grid, ipos[None, :] + t[:, None] * idir[r])
        sigma = scale * raw
        on = sigma > 0
        e = np.exp(-(sigma * h[r]))
        w = np.where(on, T[r] * (1.0 - e), 0.0)
        nn = g @ M[:3, :3]                                                            # row i: transpose(Minv3) g_i
        ln = np.linalg.norm(nn, axis=1, keepdims=True)
        nh = -nn / np.where(ln > 0, ln, 1.0)
        K[r] += w
        D[r] += w * t
        A[r] += w[:, None] * alb[None, :]
        Nn[r] += w[:, None] * nh
        T[r] = np.where(on, T[r] * e, T[r])
        running[r[on & (T[r] <= he.MIN_T)]] = False
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


def coverage_statistic(kappa_hat, kappa, n):
    """the issue's statistic over the pixels with kappa < 0.99: D = mean(kappa_hat - kappa), sigma = sqrt(sum kappa (1 - kappa) / n) / N, z = D / sigma.
    -> (z, D, pixels kept)"""
    keep = kappa < 0.99
    N = int(keep.sum())
    k = np.asarray(kappa, np.float64)[keep]
    D = float((np.asarray(kappa_hat, np.float64)[keep] - k).mean())
    sigma = float(np.sqrt((k * (1.0 - k)).sum() / n) / N)
    return D / sigma, D, N
