"""Inputs of the lookup probes (volren_amd/csrc/vr_probe.h), shared by tests/test_lookups_host.py (CPU) and tests/test_gpu_lookups.py (device):
items of four 32-bit words, whole tables and their edges.  Every generator is deterministic (fixed seeds)."""
import numpy as np

from hk_common import bits

VOXEL, TRILINEAR, MAJORANT, IMPORTANCE, TEXEL, SKY, LIGHT, TF = range(8)


def same(got, want):
    """bit for bit, NaN equal to NaN.  Not hk_common.same: any NaN equals any other, and the shapes must agree"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def first_difference(items, got, want):
    bad = ~((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(-1)
    i = int(np.nonzero(bad)[0][0])
    return "%d of %d items differ; first: item %d = %r (as float %r): got %r want %r" % (
        int(bad.sum()), len(items), i, items[i].tolist(), items[i].view(np.float32).tolist(), got[i].tolist(), want[i].tolist())


def _items(*cols):
    """columns of int32 / uint32 / float32 -> [n][4] uint32 (missing columns are 0)"""
    n = len(cols[0])
    out = np.zeros((n, 4), np.uint32)
    for k, c in enumerate(cols):
        c = np.asarray(c)
        out[:, k] = c.astype(np.float32).view(np.uint32) if c.dtype.kind == "f" else c.astype(np.int64).astype(np.uint32)
    return out


def voxel_box(extent, grid=0, ring=2):
    """every voxel of [-ring, extent + ring) on each axis (extent = (nx, ny, nz))"""
    ax = [np.arange(-ring, e + ring, dtype=np.int32) for e in extent]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return _items(np.full(x.size, grid, np.int32), x.ravel(), y.ravel(), z.ravel())


def voxel_set(n_bricks, grid=0, n_random=1 << 20, seed=11):
    """The structured set of a full-size grid: first and last voxel of the first and last brick, the brick with the highest index on each axis,
    every brick of the last z layer (its first and last voxel), one voxel of every brick of the grid, and n_random voxels drawn with a fixed seed (two voxels beyond the extent included)."""
    nbx, nby, nbz = n_bricks
    pts = []
    for b in ((0, 0, 0), (nbx - 1, nby - 1, nbz - 1), (nbx - 1, 0, 0), (0, nby - 1, 0), (0, 0, nbz - 1)):
        for o in (0, 7):
            pts.append((b[0] * 8 + o, b[1] * 8 + o, b[2] * 8 + o))
    pts = np.array(pts, np.int32)
    by, bx = np.meshgrid(np.arange(nby, dtype=np.int32), np.arange(nbx, dtype=np.int32), indexing="ij")
    layer = np.concatenate([np.stack([bx.ravel() * 8 + o, by.ravel() * 8 + o, np.full(bx.size, (nbz - 1) * 8 + o, np.int32)], 1) for o in (0, 7)])
    rs = np.random.RandomState(seed)
    rnd = np.stack([rs.randint(-2, 8 * n + 2, n_random) for n in (nbx, nby, nbz)], 1).astype(np.int32)
    # one voxel of EVERY brick (its place inside the brick varies with the brick): every brick's range -- minimum and difference -- is read
    bz, by, bx = (a.ravel() for a in np.meshgrid(np.arange(nbz, dtype=np.int64), np.arange(nby, dtype=np.int64), np.arange(nbx, dtype=np.int64), indexing="ij"))
    h = (bx * 73856093) ^ (by * 19349663) ^ (bz * 83492791)
    every = np.stack([bx * 8 + (h & 7), by * 8 + ((h >> 3) & 7), bz * 8 + ((h >> 6) & 7)], 1).astype(np.int32)
    p = np.concatenate([pts, layer, every, rnd])
    return _items(np.full(len(p), grid, np.int32), p[:, 0], p[:, 1], p[:, 2])


def trilinear_points(extent, grid=0, n=1 << 16, seed=5):
    """index-space positions: inside, exactly on voxel, cell (4) and brick (8) borders, half-voxel offsets (weights 0), just outside, far outside, NaN and inf"""
    rs = np.random.RandomState(seed)
    e = np.asarray(extent, np.float32)
    inside = (rs.uniform(0, 1, (n, 3)) * (e + 6) - 3).astype(np.float32)
    snapped = np.round(inside[: n // 4] * 2) / 2                                        # integers and half-integers
    borders = (np.round(inside[: n // 4] / 4) * 4 + rs.choice([-0.5, 0.0, 0.5, 1e-3], (n // 4, 3))).astype(np.float32)
    odd = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [-1e9, 2, 2], [3e9, 3e9, 3e9], [0.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [0, 0, 0]], np.float32)
    edge = np.concatenate([e[None] + d for d in (-0.5, 0.0, 0.5, 1.0)]).astype(np.float32)
    p = np.concatenate([inside, snapped.astype(np.float32), borders, odd, edge])
    return _items(np.full(len(p), grid, np.int32), p[:, 0], p[:, 1], p[:, 2])


def majorant_cells(n_bricks, clean=False):
    """every cell of every level 0..3 of the padded power-of-two box, one ring outside it (so: one ring outside the real extent, and one outside the
    padded box), at the cell centre and at the cell's first voxel; the general form also gets NaN, infinities and huge positions"""
    sh = [max(3, int(np.ceil(np.log2(max(n, 1))))) for n in n_bricks]
    out = []
    for mip in range(4):
        ax = [np.arange(-1, (1 << max(s - mip, 0)) + 1, dtype=np.float32) for s in sh]
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        cell = np.float32(8 << mip)
        for off in (np.float32(0.5), np.float32(0.0)):
            out.append(_items((x.ravel() + off) * cell, (y.ravel() + off) * cell, (z.ravel() + off) * cell, np.full(x.size, mip, np.int32)))
    if not clean:
        odd = np.array([[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 1, 1], [1, -np.inf, 1], [4e9, 1, 1], [-4e9, 1, 1], [-0.0, -0.0, -0.0], [-1e-30, 1, 1]], np.float32)
        for mip in range(4):
            out.append(_items(odd[:, 0], odd[:, 1], odd[:, 2], np.full(len(odd), mip, np.int32)))
    return np.concatenate(out)


def importance_all(dim=512):
    """every texel of every level, plus the ring outside each level"""
    out = []
    for mip in range(int(np.log2(dim)) + 1):
        d = dim >> mip
        y, x = np.meshgrid(np.arange(-1, d + 1, dtype=np.int32), np.arange(-1, d + 1, dtype=np.int32), indexing="ij")
        out.append(_items(x.ravel(), y.ravel(), np.full(x.size, mip, np.int32)))
    return np.concatenate(out)


def texel_points(w, h, n_random=1 << 20, seed=9):
    """every texel centre, every texel edge, u and v in {0, 1, below 0, above 1, 1 - 2^-24}, NaN / inf, and seeded random points in [-0.5, 1.5)"""
    one_m = np.float32(1.0 - 2.0 ** -24)
    us = np.concatenate([(np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w), np.arange(w + 1, dtype=np.float32) / np.float32(w)])
    vs = np.concatenate([(np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h), np.arange(h + 1, dtype=np.float32) / np.float32(h)])
    special = np.array([0.0, 1.0, -1e-3, -0.25, -1.0, -7.3, 1.0 + 1e-3, 1.25, 2.0, 9.6, one_m, np.nextafter(np.float32(0), np.float32(1))], np.float32)
    us, vs = np.concatenate([us, special]), np.concatenate([vs, special])
    if len(us) * len(vs) > (1 << 21):                    # a large map: its centres and edges crossed with each other, the special values crossed with each other
        g = np.meshgrid(vs[:2 * h + 1], us[:2 * w + 1], indexing="ij")
        u, v = np.concatenate([g[1].ravel(), np.repeat(special, len(special))]), np.concatenate([g[0].ravel(), np.tile(special, len(special))])
    else:
        g = np.meshgrid(vs, us, indexing="ij")
        u, v = g[1].ravel(), g[0].ravel()
    rs = np.random.RandomState(seed)
    r = rs.uniform(-0.5, 1.5, (n_random, 2)).astype(np.float32)
    odd = np.array([[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [0.5, -np.inf], [3e9, 0.5], [-3e9, 0.5], [0.5, 3e9]], np.float32)
    return _items(np.concatenate([u, r[:, 0], odd[:, 0]]), np.concatenate([v, r[:, 1], odd[:, 1]]))


def sky_directions(n=1 << 16, seed=4):
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [np.nan, 0, 1], [-1, 0, -0.0], [-1, 0, 1e-30], [-1, 0, -1e-30]], np.float32)
    d = np.concatenate([d, axes])
    return _items(d[:, 0], d[:, 1], d[:, 2])


def tf_densities(n=1 << 16, seed=6):
    rs = np.random.RandomState(seed)
    d = np.concatenate([rs.uniform(-0.5, 1.5, n), np.linspace(0, 1, 4097), [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1e30, -1e30]]).astype(np.float32)
    return _items(d)


# ---- light samples ----------------------------------------------------------------------------------------------------------------------------
def _levels(impmap, dim=512):
    out, off = [], 0
    d = dim
    while d >= 1:
        out.append(np.asarray(impmap[off:off + d * d], np.float32).reshape(d, d))
        off += d * d
        d >>= 1
    return out


def _thresholds(level):
    """(d, e0, e1) of every 2x2 block of one pyramid level, in float32 as the oracle computes them"""
    w0, w1, w2, w3 = level[0::2, 0::2], level[0::2, 1::2], level[1::2, 0::2], level[1::2, 1::2]
    with np.errstate(all="ignore"):
        q0, q1 = w0 + w2, w1 + w3
        return q0 / np.maximum(np.float32(1e-8), q0 + q1), w0 / q0, w1 / q1


def _warp_levels(impmap, dim=512):
    """The warp coarse to fine, in float64: for every table level the raw-draw rectangle [x0, x1] x [y0, y1] of each of its records (2^k x 2^k arrays) and the
    record's thresholds (d, e0, e1; a NaN threshold sends everything right / up: taken as 0).  After the last level: the rectangles of the base-level texels."""
    lv = _levels(impmap, dim)
    base = int(np.log2(dim))
    x0, x1 = np.zeros((1, 1)), np.ones((1, 1))
    y0, y1 = np.zeros((1, 1)), np.ones((1, 1))
    for mip in range(base - 1, -1, -1):
        d, e0, e1 = (np.clip(np.nan_to_num(t.astype(np.float64), nan=0.0), 0, 1) for t in _thresholds(lv[mip]))
        yield (x0, x1, y0, y1), (d, e0, e1)
        xm = x0 + d * (x1 - x0)
        yl, yr = y0 + e0 * (y1 - y0), y0 + e1 * (y1 - y0)
        s = x0.shape[0]
        nx0, nx1, ny0, ny1 = (np.empty((2 * s, 2 * s)) for _ in range(4))
        nx0[:, 0::2], nx1[:, 0::2] = np.repeat(x0, 2, 0), np.repeat(xm, 2, 0)
        nx0[:, 1::2], nx1[:, 1::2] = np.repeat(xm, 2, 0), np.repeat(x1, 2, 0)
        ny0[0::2, 0::2], ny1[0::2, 0::2], ny0[1::2, 0::2], ny1[1::2, 0::2] = y0, yl, yl, y1
        ny0[0::2, 1::2], ny1[0::2, 1::2], ny0[1::2, 1::2], ny1[1::2, 1::2] = y0, yr, yr, y1
        x0, x1, y0, y1 = nx0, nx1, ny0, ny1
    yield (x0, x1, y0, y1), None


def light_targeted(impmap, dim=512):
    """(a) one draw per base-level texel: the centre of the texel's preimage under the warp, from nested intervals coarse to fine in float64 (split x at
    d = q0 / max(1e-8, q0 + q1), then y at e0 = w0 / q0 or e1 = w1 / q1; a NaN threshold sends everything right / up), rounded to float32.
    Returns (items, texel x, texel y) for the texels whose interval is not empty."""
    for (x0, x1, y0, y1), thr in _warp_levels(impmap, dim):
        pass
    ok = (x1 > x0) & (y1 > y0)
    ty, tx = np.nonzero(ok)
    r0 = (0.5 * (x0 + x1))[ok].astype(np.float32)
    r1 = (0.5 * (y0 + y1))[ok].astype(np.float32)
    keep = (r0 < 1) & (r1 < 1)
    return _items(r0[keep], r1[keep]), tx[keep].astype(np.int32), ty[keep].astype(np.int32)


def _around(v, n=3):
    """float32 v and its n neighbours on either side"""
    v = np.float32(v)
    out, lo, hi = [v], v, v
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
        out += [lo, hi]
    return out


def light_thresholds(impmap, dim=512, levels=3):
    """(b) the thresholds of every record of the `levels` coarsest table levels (1 + 4 + 16 records), and r = 0 and r = 1 - 2^-24 on both axes.
    The coarsest record compares its thresholds with the raw draw: the draws exactly on, one ulp below and one ulp above each are in the set.  A deeper
    record compares them with the RESCALED coordinate, so its thresholds are mapped back to raw draws through the parent rectangles (as light_targeted does, in
    float64) and the set holds the float32 draws around that point, three on either side, with the other axis inside the record's rectangle (for e0 / e1: in the
    left / right part): the nearest draws that float32 can place on either side of such a threshold -- the rescaled coordinate takes only some float32 values, so
    "exactly on" is hit there only when the chain of roundings allows it."""
    lv = _levels(impmap, dim)
    base = int(np.log2(dim))
    one_m = np.float32(1.0 - 2.0 ** -24)
    vals = [np.float32(0.0), one_m]
    for mip in range(base - 1, base - 1 - levels, -1):
        for t in _thresholds(lv[mip]):
            t = t[np.isfinite(t)].ravel()
            vals += [t, np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))]
    v = np.unique(np.concatenate([np.atleast_1d(x).astype(np.float32) for x in vals]))
    v = v[(v >= 0) & (v < 1)]
    g = np.meshgrid(v, v, indexing="ij")
    r0, r1 = [g[0].ravel()], [g[1].ravel()]
    for k, ((x0, x1, y0, y1), thr) in enumerate(_warp_levels(impmap, dim)):
        if k >= levels or thr is None:
            break
        d, e0, e1 = thr
        for cy in range(x0.shape[0]):
            for cx in range(x0.shape[1]):
                a, b, c, e = x0[cy, cx], x1[cy, cx], y0[cy, cx], y1[cy, cx]
                xm = a + d[cy, cx] * (b - a)
                xs = _around(xm) + [np.float32(0.5 * (a + xm)), np.float32(0.5 * (xm + b))]
                ys = _around(c + e0[cy, cx] * (e - c)) + _around(c + e1[cy, cx] * (e - c)) + [np.float32(0.5 * (c + e)), np.float32(0.0), one_m]
                gx, gy = np.meshgrid(np.array(xs + [np.float32(0.0), one_m], np.float32), np.array(ys, np.float32), indexing="ij")
                r0.append(gx.ravel())
                r1.append(gy.ravel())
    r0, r1 = np.concatenate(r0), np.concatenate(r1)
    keep = (r0 >= 0) & (r0 < 1) & (r1 >= 0) & (r1 < 1)
    return _items(r0[keep], r1[keep])


def light_lattice(n=1024):
    """(c) a regular n x n lattice in [0, 1)"""
    a = (np.arange(n, dtype=np.float32) + np.float32(0.5)) / np.float32(n)
    g = np.meshgrid(a, a, indexing="ij")
    return _items(g[1].ravel(), g[0].ravel())


# ---- environment maps ---------------------------------------------------------------------------------------------------------------------------
def rgbe_map(w, h):
    """an exact-RGBE map (the generator of test_small_environment_maps_in_compact_form): image rows, top first"""
    rs = np.random.RandomState(w * 100 + h)
    m = rs.randint(0, 256, (h, w, 3)).astype(np.float32)
    m[..., 0] = rs.randint(128, 256, (h, w))
    m[..., 1:] = np.minimum(m[..., 1:], m[..., :1])
    env = (m * np.exp2(rs.randint(-12, 2, (h, w, 1)).astype(np.float32))).astype(np.float32)
    env[0, 0] = 0.0
    return env


def nudged(env):
    """the same map with one texel off the RGBE grid: it keeps its float form"""
    e = env.copy()
    e[-1, -1, 1] = np.float32(1.0 / 3.0)
    return e


def dark_patch_map():
    """the map of test_environment_whose_warp_table_fails_the_division_check: thresholds below 2^-76 (env_div_safe = 0)"""
    rs = np.random.RandomState(3)
    env = rs.uniform(0.2, 1.0, (8, 16, 3)).astype(np.float32)
    env[2:5, 4:7] = 1e-30
    env[4, 11] = 0.0
    return env


def one_lit_map(w=16, h=8):
    env = np.zeros((h, w, 3), np.float32)
    env[h // 3, (2 * w) // 3] = (3.0, 2.0, 1.0)
    return env
