"""Inputs of the per-path probes (volren_amd/csrc/vr_path_probe.h), shared by tests/test_path_probes_host.py (CPU) and tests/test_gpu_path_probes.py (device):
item arrays of 32-bit words in the layouts oracle/volren_oracle.h states for orc_batch_rng ... orc_batch_segment, and the scenes the segment sets run on.
Every generator is deterministic (fixed seeds); all sizes are the ones the tests run."""
import numpy as np

import scenes

RNG, CAMERA, BOX, PHASE, DDA, SEGMENT = range(6)
KIND_NAMES = ("rng", "camera", "box", "phase", "dda_step", "segment")
M32 = 0xFFFFFFFF
LCG_A, LCG_C = 1664525, 1013904223
LCG_A_INV = pow(LCG_A, -1, 1 << 32)
ONE_M = np.float32(1.0 - 2.0 ** -24)

# which words of an item / a result are floats (the others are integers): for messages
IN_FLOAT = ((), (), range(6), range(9), range(6), range(6))
OUT_FLOAT = ((0,), (0, 1, 2), (1, 2), range(5), (0,), (1, 2, 6, 7, 8, 9, 10, 11, 12))
SEGMENT_COMPARED = 13                  # the oracle's words; word 13 of the product's result is seg_clean


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(kind, got, want):
    """word for word; a float word that is NaN on both sides may be any NaN (lookup_cases.same on those words)"""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    if got.shape != want.shape:
        return False
    eq = got == want
    for k in OUT_FLOAT[kind]:
        if k < got.shape[1]:
            eq[:, k] |= np.isnan(got[:, k].view(np.float32)) & np.isnan(want[:, k].view(np.float32))
    return bool(eq.all())


def _decode(words, floats):
    return [float(np.uint32(w).view(np.float32)) if k in floats else int(np.int64(w)) for k, w in enumerate(words)]


def first_difference(kind, items, got, want):
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    eq = got == want
    for k in OUT_FLOAT[kind]:
        if k < got.shape[1]:
            eq[:, k] |= np.isnan(got[:, k].view(np.float32)) & np.isnan(want[:, k].view(np.float32))
    bad = ~eq.all(1)
    i = int(np.nonzero(bad)[0][0])
    return "%s: %d of %d items differ; first: item %d = %r (words %s): got %r want %r" % (
        KIND_NAMES[kind], int(bad.sum()), len(items), i, _decode(items[i], IN_FLOAT[kind]), [hex(int(w)) for w in items[i]],
        _decode(got[i], OUT_FLOAT[kind]), _decode(want[i], OUT_FLOAT[kind]))


def _words(*cols):
    """columns of integers or float32 -> [n][len(cols)] uint32"""
    n = max(np.size(c) for c in cols)
    out = np.zeros((n, len(cols)), np.uint32)
    for k, c in enumerate(cols):
        c = np.asarray(c)
        out[:, k] = fbits(c.astype(np.float32)) if c.dtype.kind == "f" else (c.astype(np.int64) & M32).astype(np.uint32)
    return out


# ---- RNG --------------------------------------------------------------------------------------------------------------------------------------
def states_with_first_draw(low24):
    """the 256 LCG states whose NEXT draw has the 24 bits `low24`: the recurrence solved backwards, s = (k 2^24 + low24 - c) a^-1 mod 2^32"""
    k = np.arange(256, dtype=np.uint64)
    return ((((k << np.uint64(24)) + np.uint64(low24) + np.uint64((1 << 32) - LCG_C)) * np.uint64(LCG_A_INV)) & np.uint64(M32)).astype(np.uint32)


def np_tea32(v0, v1):
    """common.glsl:40-52 in NumPy (the restatement of tests/test_seed_table_host.py, vectorised): 32 rounds, returns v0"""
    v0, v1 = np.asarray(v0, np.uint64) & np.uint64(M32), np.asarray(v1, np.uint64) & np.uint64(M32)
    m, s0 = np.uint64(M32), np.uint64(0)
    for _ in range(32):
        s0 = (s0 + np.uint64(0x9E3779B9)) & m
        v0 = (v0 + ((((v1 << np.uint64(4)) & m) + np.uint64(0xA341316C)) & m ^ ((v1 + s0) & m) ^ (((v1 >> np.uint64(5)) + np.uint64(0xC8013EA4)) & m))) & m
        v1 = (v1 + ((((v0 << np.uint64(4)) & m) + np.uint64(0xAD90777D)) & m ^ ((v0 + s0) & m) ^ (((v0 >> np.uint64(5)) + np.uint64(0x7E95761E)) & m))) & m
    return v0.astype(np.uint32)


def np_rng_reference(items):
    """the five words of the RNG probe in NumPy integer arithmetic: a second reference beside the oracle"""
    it = items.astype(np.uint64)
    m = np.uint64(M32)
    s1 = (it[:, 0] * np.uint64(LCG_A) + np.uint64(LCG_C)) & m
    draw = ((s1 & np.uint64(0xFFFFFF)).astype(np.float32) / np.float32(16777216.0)).astype(np.float32)
    s9 = it[:, 0]
    for _ in range(9):
        s9 = (s9 * np.uint64(LCG_A) + np.uint64(LCG_C)) & m
    pix = (it[:, 6] * it[:, 4] + it[:, 5]) & m
    return np.stack([fbits(draw), s1.astype(np.uint32), s9.astype(np.uint32), np_tea32(it[:, 1], it[:, 2]), np_tea32((it[:, 3] * pix) & m, it[:, 7])], 1)


def seed_pixels():
    """(seed, W, px, py, smp): seeds 0, 1, 42, -7; W = 1 and 70 at every pixel of a 1 x 64 and a 70 x 37 frame, W = 1031 and 46341 (py W + px wraps) at the
    corners of a square frame; samples 1, 2, 2^24 + 1"""
    rows = []
    for w, h in ((1, 64), (70, 37)):
        py, px = (a.ravel() for a in np.meshgrid(np.arange(h), np.arange(w), indexing="ij"))
        rows.append(np.stack([np.full(px.size, w), px, py], 1))
    for w in (1031, 46341):
        rows.append(np.array([[w, x, y] for x in (0, w - 1) for y in (0, w - 1)]))
    pix = np.concatenate(rows)
    out = [np.concatenate([np.full((len(pix), 1), seed), pix, np.full((len(pix), 1), smp)], 1) for seed in (0, 1, 42, -7) for smp in (1, 2, (1 << 24) + 1)]
    return np.concatenate(out).astype(np.int64)


def rng_items():
    """2^20 strided states plus 0, 1, 2^32 - 1 and the states whose next draw is 0 and 1 - 2^-24; tea32 on a 1024 x 1024 lattice plus the corners; the path seeds
    of seed_pixels().  One item carries one of each; the shorter lists repeat."""
    n = 1 << 20
    i = np.arange(n, dtype=np.uint64)
    states = np.concatenate([((i * np.uint64(4099)) & np.uint64(M32)).astype(np.uint32), np.array([0, 1, M32], np.uint32), states_with_first_draw(0), states_with_first_draw(0xFFFFFF)])
    a = ((np.arange(1024, dtype=np.uint64) * np.uint64(0x00400801)) & np.uint64(M32)).astype(np.uint32)
    v1, v0 = (g.ravel() for g in np.meshgrid(a, a, indexing="ij"))
    corners = np.array([[0, 0], [0, M32], [M32, 0], [M32, M32]], np.uint32)
    v0, v1 = np.concatenate([v0, corners[:, 0]]), np.concatenate([v1, corners[:, 1]])
    sp = seed_pixels()
    m = max(len(states), len(v0), len(sp))
    k = np.arange(m)
    sp = sp[k % len(sp)]
    return _words(states[k % len(states)], v0[k % len(v0)], v1[k % len(v1)], sp[:, 0], sp[:, 1], sp[:, 2], sp[:, 3], sp[:, 4])


# ---- camera -----------------------------------------------------------------------------------------------------------------------------------
CAMERA_FRAMES = ((1, 1), (2, 3), (70, 37), (4096, 1), (1, 4096))
# c2's camera; the top-down and the inside camera of tests/test_gpu_parity.py FLAG_VARIANTS; fov 0.003 from 3e4 away (its camera_very_far); fov 0 and 180
CAMERAS = {
    "c2": dict(),
    "top_down": dict(cam_pos=(0.0, 2.0, 0.0), cam_dir=(0.0, -1.0, 0.001), cam_up=(0.0, 0.0, 1.0)),
    "inside_fov95": dict(cam_pos=(0.0, -0.2, 0.05), cam_dir=(0.3, 1.0, 0.1), cam_fov=95.0),
    "far_fov0.003": dict(cam_pos=(3.0e4, 0.5e4, 2.0e4), cam_dir=(-0.8241634368896484, -0.1373605728149414, -0.5494422912597656), cam_fov=0.003),
    "fov0": dict(cam_fov=0.0),
    "fov180": dict(cam_fov=180.0),
}


def camera_items(w, h):
    """every pixel of a small frame, the corners of a large one; samples 1, 2 and 2^24 + 1"""
    if w * h <= 4096 and min(w, h) > 1 or w * h == 1:
        py, px = (a.ravel() for a in np.meshgrid(np.arange(h), np.arange(w), indexing="ij"))
    else:
        px, py = np.array([0, w - 1, 0, w - 1]), np.array([0, 0, h - 1, h - 1])
    out = [_words(px, py, np.full(px.size, smp), np.zeros(px.size, np.int64)) for smp in (1, 2, (1 << 24) + 1)]
    return np.concatenate(out)


def camera_scene(is_oracle, camera, w, h, seed=42):
    r = scenes.oracle_scene("c2", w, h) if is_oracle else scenes.hip_scene("c2", w, h)
    for k, v in CAMERAS[camera].items():
        setattr(r, k, v)
    r.seed = seed
    return r


# ---- box --------------------------------------------------------------------------------------------------------------------------------------
def _unit(rs, n):
    d = rs.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _axes_signed_zeros():
    """the 6 axes, the two other components +0 and -0 in every combination: 24 directions"""
    out = []
    for a in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    d = [z1, z2]
                    d.insert(a, s)
                    out.append(d)
    return np.array(out, np.float32)


def _diagonals():
    """the 12 face diagonals and the 8 space diagonals, not normalised in float64 first: components exactly equal in modulus"""
    out = []
    for a in range(3):
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                d = [s1, s2]
                d.insert(a, 0.0)
                out.append(d)
    out += [[sx, sy, sz] for sx in (1.0, -1.0) for sy in (1.0, -1.0) for sz in (1.0, -1.0)]
    d = np.array(out, np.float64)
    n = np.float32(1.0) / np.sqrt((d * d).sum(1)).astype(np.float32)
    return (d.astype(np.float32) * n[:, None]).astype(np.float32)


ODD = np.array([1e-20, 1e-38, 1e-42, 1e30, np.nan, np.inf, -np.inf], np.float32)


def box_directions(seed=21, n_random=1 << 12):
    base = np.concatenate([_axes_signed_zeros(), _diagonals(), _unit(np.random.RandomState(seed), n_random)])
    out = [base, np.zeros((1, 3), np.float32)]
    rs = np.random.RandomState(seed + 1)
    comp = rs.randint(0, 3, len(base))
    for v in ODD:                                   # each direction with one component replaced
        d = base.copy()
        d[np.arange(len(base)), comp] = v
        out.append(d)
    return np.concatenate(out)


def _ulp_around(v):
    v = np.asarray(v, np.float32)
    return np.stack([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))], -1)


def box_origins(bmin, bmax):
    """a 9^3 lattice over the box grown by one half (it holds the box's faces, edges and corners exactly: coordinates 2 and 6 of 0..8), and every lattice point that
    lies on the box's surface again with each coordinate one ulp down and up"""
    bmin, bmax = np.asarray(bmin, np.float32), np.asarray(bmax, np.float32)
    ax = []
    for a in range(3):
        lo, hi = np.float64(bmin[a]), np.float64(bmax[a])
        t = (np.arange(9) - 2) / 4.0                # -0.5 ... 1.5 in steps of 0.25
        c = (lo + t * (hi - lo)).astype(np.float32)
        c[2], c[6] = bmin[a], bmax[a]               # exactly
        ax.append(c)
    z, y, x = (g.ravel() for g in np.meshgrid(ax[2], ax[1], ax[0], indexing="ij"))
    lattice = np.stack([x, y, z], 1)
    on = ((lattice == bmin) | (lattice == bmax)).any(1) & ((lattice >= bmin) & (lattice <= bmax)).all(1)
    surf = lattice[on]
    near = [surf]
    for a in range(3):
        for step in (-np.inf, np.inf):
            p = surf.copy()
            p[:, a] = np.nextafter(p[:, a], np.float32(step))
            near.append(p)
    return lattice, np.concatenate(near)


def box_items(bmin, bmax, seed=22, limit=1 << 17):
    """the lattice x the structured directions, the surface points (+- 1 ulp) x every direction, thinned to `limit` items by a fixed permutation that keeps the
    structured part whole"""
    lattice, surf = box_origins(bmin, bmax)
    dirs = box_directions()
    structured = np.concatenate([_axes_signed_zeros(), _diagonals(), np.zeros((1, 3), np.float32)])
    rs = np.random.RandomState(seed)

    def cross(p, d):
        return np.concatenate([np.repeat(p, len(d), 0), np.tile(d, (len(p), 1))], 1)
    a = cross(surf, structured)
    b = cross(lattice, structured)
    n_rest = max(0, limit - len(a) - len(b))
    pi, di = rs.randint(0, len(surf), n_rest // 2), rs.randint(0, len(dirs), n_rest // 2)
    c = np.concatenate([surf[pi], dirs[di]], 1)
    pi, di = rs.randint(0, len(lattice), n_rest - n_rest // 2), rs.randint(0, len(dirs), n_rest - n_rest // 2)
    d = np.concatenate([lattice[pi], dirs[di]], 1)
    out = np.concatenate([a, b, c, d])[:limit]
    return fbits(out).copy()


CROP = dict(vol_clip_min=(0.2, 0.1, 0.0), vol_clip_max=(0.9, 0.6, 1.0))       # the `crop` variant of tests/test_gpu_parity.py FLAG_VARIANTS


# ---- phase ------------------------------------------------------------------------------------------------------------------------------------
PHASE_G = np.array([0.0] + [s * v for v in (9.9e-5, 1e-4, 1.1e-4, 0.3, 0.7, 0.999, 1.0) for s in (1, -1)], np.float32)


def phase_directions(seed=31):
    d = [_axes_signed_zeros()[::4]]                                                          # the 6 axes
    e = [[sx * a, sy * a, z] for a in (1.0, 0.5, 0.6) for sx in (1, -1) for sy in (1, -1) for z in (0.0, 0.3, -0.8)]      # |x| == |y| exactly
    d.append(np.array(e, np.float32))
    d.append(np.array([[zx, zy, s] for zx in (0.0, -0.0) for zy in (0.0, -0.0) for s in (1.0, -1.0)], np.float32))       # (0, 0, +-1) with +-0 in x and y
    d.append(_unit(np.random.RandomState(seed), 256))
    return np.concatenate(d)


def phase_items():
    """words: cos, g, dir, r0, r1, a, b.  phase_hg: every g x 4097 cosines; sample_phase_hg: every g x every direction x the six special draws on both axes, and
    every g x 16 directions x a 64 x 64 lattice; power_heuristic: the pairs over {0, 1e-30, 1e-20, 1, 1e19, 1e20, inf}"""
    cos = np.linspace(-1.0, 1.0, 4097).astype(np.float32)
    dirs = phase_directions()
    special = np.array([0.0, 2.0 ** -24, 0.25, 0.5, 0.75, ONE_M], np.float32)
    rows = []
    g, c = (a.ravel() for a in np.meshgrid(PHASE_G, cos, indexing="ij"))
    z = np.zeros(g.size, np.float32)
    rows.append(np.stack([c, g, z + 1, z, z, z, z, z, z], 1))
    gi, di, r0, r1 = (a.ravel() for a in np.meshgrid(np.arange(len(PHASE_G)), np.arange(len(dirs)), special, special, indexing="ij"))
    z = np.zeros(gi.size, np.float32)
    rows.append(np.concatenate([z[:, None], PHASE_G[gi][:, None], dirs[di], r0[:, None], r1[:, None], z[:, None], z[:, None]], 1))
    lat = ((np.arange(64) + 0.5) / 64.0).astype(np.float32)
    some = dirs[np.linspace(0, len(dirs) - 1, 16).astype(int)]
    gi, di, r0, r1 = (a.ravel() for a in np.meshgrid(np.arange(len(PHASE_G)), np.arange(len(some)), lat, lat, indexing="ij"))
    z = np.zeros(gi.size, np.float32)
    rows.append(np.concatenate([z[:, None], PHASE_G[gi][:, None], some[di], r0[:, None], r1[:, None], z[:, None], z[:, None]], 1))
    v = np.array([0.0, 1e-30, 1e-20, 1.0, 1e19, 1e20, np.inf], np.float32)
    a, b = (x.ravel() for x in np.meshgrid(v, v, indexing="ij"))
    z = np.zeros(a.size, np.float32)
    rows.append(np.stack([z, z, z + 1, z, z, z, z, a, b], 1))
    return fbits(np.concatenate(rows).astype(np.float32)).copy()


# ---- DDA step ---------------------------------------------------------------------------------------------------------------------------------
def dda_items(clean=False):
    """points on voxel, brick and 2-, 4-, 8-brick boundaries of a 64^3-voxel index space, each also +- 1 ulp and +- 0.5, x reciprocal directions of every sign
    pattern -- finite ones, +-inf (a zero direction component), +-0 (an infinite one) and, in the general form only, NaN -- x mips 0..3.  clean: no NaN (the CLEAN form's contract)"""
    b = np.array([0.0, 1.0, 7.0, 8.0, 9.0, 16.0, 24.0, 32.0, 33.0, 48.0, 63.0, 64.0], np.float32)
    pts = np.unique(np.concatenate([_ulp_around(b).ravel(), b - np.float32(0.5), b + np.float32(0.5), np.array([-0.0, -1.0, -8.0, 65.0, 72.0], np.float32)]).view(np.uint32)).view(np.float32)
    rs = np.random.RandomState(41)
    n = 1 << 14
    p = pts[rs.randint(0, len(pts), (n, 3))]
    p[: len(pts)] = np.stack([pts, pts[::-1], np.roll(pts, 5)], 1)
    # (0: the reciprocal of an infinite component, +0 or -0 -- the one place where stepDDA's `inv_dir >= 0` and a `> 0` part: the candidate's sign of zero)
    # A clean segment's |idir| is below 2^20 on every axis (vr_trace.h seg_clean), its reciprocal above 2^-20 or infinite: no zero there
    mag = np.array([1.0, 1.5, 0.037, 250.0, np.inf, 3e-5, 2e6], np.float32)
    if not clean:
        mag = np.concatenate([mag, np.array([0.0, np.nan], np.float32)])
    ri = mag[rs.randint(0, len(mag), (n, 3))] * rs.choice(np.array([1.0, -1.0], np.float32), (n, 3))
    k = np.arange(n)
    for a in range(3):                                # every sign pattern is there by construction of the first 8 x 8 rows as well
        ri[: 64, a] = np.abs(ri[: 64, a]) * np.where((k[:64] >> a) & 1, -1.0, 1.0)
    mip = k % 4
    if not clean:
        odd = np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [3e9, 1, 1], [-3e9, 1, 1]], np.float32)
        p[64:64 + len(odd)] = odd
    return np.concatenate([fbits(p), fbits(ri.astype(np.float32)), mip[:, None].astype(np.uint32)], 1)


# ---- segments ---------------------------------------------------------------------------------------------------------------------------------
def _mat_point(m, p):
    """column-major 4x4 times (p, 1), float64"""
    m = np.asarray(m, np.float64).reshape(4, 4).T
    return p @ m[:3, :3].T + m[:3, 3]


def _replace_component(d, rs, values):
    d = d.copy()
    d[np.arange(len(d)), rs.randint(0, 3, len(d))] = values[rs.randint(0, len(values), len(d))]
    return d


def _aimed(rs, n, bmin, bmax, radius):
    c, ext = 0.5 * (bmin + bmax), bmax - bmin
    diag = np.sqrt((ext * ext).sum())
    o = c + radius * diag * _unit(rs, n).astype(np.float64)
    target = bmin + rs.uniform(0, 1, (n, 3)) * ext
    d = target - o
    return o.astype(np.float32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def segment_rays(params, index_extent, seed=51, n_aimed=1 << 12, n_inside=1 << 13):
    """The ray classes of one scene, as a dict name -> (origins, directions) in world space, float32.  params: the oracle's uniform block (box, transforms);
    index_extent: the density grid's extent in voxels."""
    rs = np.random.RandomState(seed)
    bmin, bmax = np.array(params.vol_bb_min[:], np.float64), np.array(params.vol_bb_max[:], np.float64)
    ext = bmax - bmin
    sets = {}
    # 1. aimed at the box from three, 1e3 and 3e4 diagonals out (the last: not clean)
    parts = [_aimed(rs, n_aimed, bmin, bmax, 3.0), _aimed(rs, 1 << 9, bmin, bmax, 1e3), _aimed(rs, 1 << 9, bmin, bmax, 3e4)]
    sets["aimed"] = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
    # 2. scatter and shadow segments: uniform origin inside the box, uniform direction
    sets["inside"] = ((bmin + rs.uniform(0, 1, (n_inside, 3)) * ext).astype(np.float32), _unit(rs, n_inside))
    # 3. origins on voxel / brick / coarse-cell boundaries of the index space, through the scene's transform, +- 1 ulp per coordinate
    n = 1 << 11
    gran = np.array([1, 8, 16, 32, 64])[rs.randint(0, 5, (n, 3))]
    idx = gran * np.floor(rs.uniform(0, 1, (n, 3)) * (np.asarray(index_extent) // gran + 1))
    o = _mat_point(params.vol_density_transform[:], idx).astype(np.float32)
    step = rs.randint(-1, 2, (n, 3))
    o = np.where(step < 0, np.nextafter(o, np.float32(-np.inf)), np.where(step > 0, np.nextafter(o, np.float32(np.inf)), o)).astype(np.float32)
    structured = np.concatenate([_axes_signed_zeros(), _diagonals()])
    sets["boundary"] = (o, structured[np.arange(n) % len(structured)])
    # 4. grazing: in a face's plane, along an edge, through a corner, from a face inwards and outwards
    n = 1 << 10
    k = np.arange(n)
    axis, side, cls = k % 3, (k // 3) % 2, (k // 6) % 5
    o = bmin + rs.uniform(-0.25, 1.25, (n, 3)) * ext
    face = np.where(side == 0, bmin[axis], bmax[axis])
    o[k, axis] = face                                             # on the face's plane
    d = _unit(rs, n).astype(np.float64)
    d[cls == 0, :] = np.where(np.arange(3)[None, :] == axis[cls == 0, None], 0.0, d[cls == 0, :])      # in the plane
    a2 = (axis + 1) % 3
    edge = cls == 1                                               # along an edge: two coordinates on the box, direction along the third
    o[edge, a2[edge]] = np.where(side[edge] == 0, bmin[a2[edge]], bmax[a2[edge]])
    d[edge, :] = np.where(np.arange(3)[None, :] == ((axis[edge] + 2) % 3)[:, None], np.where(k[edge, None] & 64, -1.0, 1.0), 0.0)
    corner = cls == 2                                             # through a corner: from outside along a diagonal
    cpt = np.where((k[corner, None] >> np.arange(3)[None, :] + 3) & 1, bmax, bmin)
    dd = _diagonals()[12 + k[corner] % 8].astype(np.float64)
    o[corner] = cpt - dd * rs.uniform(0.5, 2.0, (corner.sum(), 1))
    d[corner] = dd
    inner = bmin + rs.uniform(0.02, 0.98, (n, 3)) * ext
    for c, sgn in ((3, 1.0), (4, -1.0)):                          # from a face's interior inwards / outwards along its normal
        m = cls == c                                              # (from a point that lies on a second face as well the reference's segment is unbounded: stall_rays)
        o[m] = inner[m]
        o[m, axis[m]] = face[m]
        d[m, :] = np.where(np.arange(3)[None, :] == axis[m, None], np.where(side[m, None] == 0, sgn, -sgn), 0.0)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    sets["grazing"] = (o.astype(np.float32), (d / np.where(nrm > 0, nrm, 1.0)).astype(np.float32))
    # 5. one direction component tiny
    n = 1 << 10
    a_o, a_d = _aimed(rs, n // 2, bmin, bmax, 3.0)
    i_o, i_d = (bmin + rs.uniform(0, 1, (n // 2, 3)) * ext).astype(np.float32), _unit(rs, n // 2)
    o, d = np.concatenate([a_o, i_o]), np.concatenate([a_d, i_d])
    sets["tiny_component"] = (o, _replace_component(d, rs, np.array([1e-20, -1e-20, 1e-30, 1e-38, 1e-42, -1e-42], np.float32)))
    # 6. direction lengths 0.25, 4, 1e3, 1e12
    a_o, a_d = _aimed(rs, n // 2, bmin, bmax, 3.0)
    i_o, i_d = (bmin + rs.uniform(0, 1, (n // 2, 3)) * ext).astype(np.float32), _unit(rs, n // 2)
    o, d = np.concatenate([a_o, i_o]), np.concatenate([a_d, i_d])
    sets["lengths"] = (o, (d * np.array([0.25, 4.0, 1e3, 1e12], np.float32)[np.arange(n) % 4][:, None]).astype(np.float32))
    # 7. NaN / +-inf / zero directions and NaN origins
    n = 1 << 8
    o, d = (bmin + rs.uniform(-0.5, 1.5, (n, 3)) * ext).astype(np.float32), _unit(rs, n)
    d[: n // 2] = _replace_component(d[: n // 2], rs, np.array([np.nan, np.inf, -np.inf], np.float32))
    d[n // 2: 3 * n // 4] = 0.0
    d[n // 2: 3 * n // 4: 2, 1] = -0.0
    o[3 * n // 4:] = _replace_component(o[3 * n // 4:], rs, np.array([np.nan], np.float32))
    sets["not_finite"] = (o, d)
    return sets


def stall_rays(params, seed=52):
    """the rays that do not end, or not within the budget: origins 1e6 box diagonals out, direction lengths 1e-12 and 1e-3, and axis directions from a point on
    two faces at once -- in the plane of the second face 0 * inf makes the box test's far end +inf, and the reference's loop walks on outside the volume -- for
    the bounded forms only.  64 rays."""
    rs = np.random.RandomState(seed)
    bmin, bmax = np.array(params.vol_bb_min[:], np.float64), np.array(params.vol_bb_max[:], np.float64)
    a_o, a_d = _aimed(rs, 16, bmin, bmax, 1e6)
    i_o, i_d = (bmin + rs.uniform(0, 1, (32, 3)) * (bmax - bmin)).astype(np.float32), _unit(rs, 32)
    i_d[:16] *= np.float32(1e-12)
    i_d[16:] *= np.float32(1e-3)
    k = np.arange(16)
    e_o = bmin + rs.uniform(0.02, 0.98, (16, 3)) * (bmax - bmin)
    axis, second = k % 3, (k % 3 + 1 + (k // 3) % 2) % 3
    e_o[k, axis] = np.where(k & 1, bmax[axis], bmin[axis])
    e_o[k, second] = np.where(k & 2, bmax[second], bmin[second])
    e_d = np.where(np.arange(3)[None, :] == axis[:, None], np.where(k[:, None] & 4, -1.0, 1.0), 0.0)
    return np.concatenate([a_o, i_o, e_o.astype(np.float32)]), np.concatenate([a_d, i_d, e_d.astype(np.float32)])


def _segment_items(o, d, states):
    """every ray x every state x both kinds"""
    n, k = len(o), len(states)
    ray = np.repeat(np.arange(n), 2 * k)
    st = np.tile(np.repeat(np.asarray(states, np.uint32), 2), n)
    kind = np.tile(np.array([0, 1], np.uint32), n * k)
    return np.concatenate([fbits(o[ray]), fbits(d[ray]), st[:, None], kind[:, None]], 1)


def segment_sets(params, index_extent, thin=1):
    """name -> items of the compared sets 1. - 8. of one scene: per ray two seeded RNG states and both kinds; `inside` and `boundary` again with the states whose
    first draw is 0 and 1 - 2^-24.  thin: divides the sizes of the random sets (aimed, inside), never the edge sets"""
    rays = segment_rays(params, index_extent, n_aimed=(1 << 12) // thin, n_inside=(1 << 13) // thin)
    rs = np.random.RandomState(53)
    out = {}
    for name, (o, d) in rays.items():
        st = rs.randint(0, 1 << 32, (len(o), 2), dtype=np.uint64).astype(np.uint32)
        a = _segment_items(o, d, [0, 0])
        a[:, 6] = np.repeat(st.ravel(), 2)
        out[name] = a
    zero, top = states_with_first_draw(0), states_with_first_draw(0xFFFFFF)
    for name in ("inside", "boundary"):
        o, d = rays[name]
        a = _segment_items(o, d, [0, 0])
        n = len(a) // 4
        a[:, 6] = np.repeat(np.stack([zero[np.arange(n) % 256], top[np.arange(n) % 256]], 1).ravel(), 2)
        out[name + "_first_draw"] = a
    # ... and `inside` with first draws of 2 x 2^-24 and 16 x 2^-24: free flights of 1.2e-7 and 9.5e-7, short enough to collide in the thinnest medium the kernels of
    # one scene kind take (density scale 2^-16), and -- unlike the 256 states of one first draw among themselves -- with different later draws from one to the other
    o, d = rays["inside"]
    a = _segment_items(o, d, [0, 0])
    n = len(a) // 4
    two, sixteen = states_with_first_draw(2), states_with_first_draw(16)
    a[:, 6] = np.repeat(np.stack([two[np.arange(n) % 256], sixteen[np.arange(n) % 256]], 1).ravel(), 2)
    out["inside_small_draw"] = a
    return out


def stall_items(params):
    o, d = stall_rays(params)
    return _segment_items(o, d, [12345, 0x9E3779B9])


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
# name -> (what is set after scenes.configure, the forms the scene serves, host-scene flags (hk_path), thin).  All renderers are 16 x 16: the probes ignore the frame.
HS_MAJ_BLOCKED, HS_NO_FLOAT_ATLAS, HS_PAIR = 1, 2, 8
ALL_SETS = ("aimed", "inside", "boundary", "grazing", "tiny_component", "lengths", "not_finite", "inside_first_draw", "boundary_first_draw", "inside_small_draw")
# over_budget: the classes of which, on that scene, the ORACLE leaves more than 1 % unfinished within its budget.  They are out of the compared sets -- the budget
# condition of tests/test_path_probes_host.py does not cover them -- and go through the bounded forms like the stall set: compared where the oracle finishes.
#   * density scale 2^24: an empty voxel inside a brick whose range is not empty is crossed in steps of tau / majorant ~ 1e-7: every class runs out (12 ... 50 %);
#   * `boundary` on c4:64 and on the brick crop: 1.0 ... 2.6 % -- index coordinate 0 or the extent puts the origin on a box face, and an axis direction in that
#     face's plane gives the box test 0 * inf: the far end is +inf and the reference's loop walks on outside the volume (the rays of stall_rays' last class);
#   * `not_finite` under the global-majorant pair: 2.7 % -- an infinite far end with a finite ray parameter.
# thin_medium: at density scales 2^-16 and 2^-17 a segment collides only on a very short free flight -- a first draw of a few 2^-24 (the *_first_draw and
#       *_small_draw sets) -- and the draw after a null collision is long again: tests/test_path_probes_host.py states what follows for the DDA levels.
SEGMENT_SCENES = {
    "c2": dict(base="c2", forms=(0, 1, 6)),
    "c2-scale-2^-16": dict(base="c2", density_scale=2.0 ** -16, forms=(0, 1, 6), thin_medium=True),
    "c2-scale-2^24": dict(base="c2", density_scale=2.0 ** 24, forms=(0, 1, 6), over_budget=ALL_SETS, thin=4),
    "c2-scale-2^-17": dict(base="c2", density_scale=2.0 ** -17, forms=(6,), thin_medium=True),
    "c3": dict(base="c3", forms=(0, 1, 6)),
    "c3-byte-atlas": dict(base="c3", float_atlas=0, forms=(0, 1, 6)),
    "c4:64": dict(base="c4:64", forms=(2, 3, 6), over_budget=("boundary",)),
    "c5:32-linear": dict(base="c5:32", layout=0, forms=(4, 6)),
    "c5:32-blocked": dict(base="c5:32", layout=1, forms=(5, 6)),
    "emission-other-layout-linear": dict(base="emission40", layout=0, forms=(6,)),
    "emission-other-layout-blocked": dict(base="emission40", layout=1, forms=(6,)),
    "ragged-5x3x7": dict(base="ragged", forms=(0, 1, 6), over_budget=("boundary", "boundary_first_draw")),
    "c2-global": dict(base="c2", integrator=1, forms=(6,), over_budget=("not_finite",)),
    "c3-global": dict(base="c3", integrator=1, forms=(6,), over_budget=("not_finite",)),
}
STATUS_WORD, BUDGET_CAP = 0, 0.01


def _emission40(is_oracle):
    """density 40^3 and temperature 40 x 40 x 72 (tests/test_gpu_lookups.py test_emission_grid_with_another_brick_layout): no paired atlas"""
    import encoder_ref
    dens = scenes.synthetic_density(40)
    temp = np.clip(dens * 0.2 + 0.1 * scenes.synthetic_density(40, seed=99), 0, None).astype(np.float32)
    temp = np.concatenate([temp, temp[:, :, :32]], 2)
    if is_oracle:
        from oracle import binding as ob
        gd, gt = encoder_ref.encode(dens), encoder_ref.encode(temp)
        gd.extent = (40, 40, 40); gd.c.extent[:] = gd.extent
        gt.extent = (72, 40, 40); gt.c.extent[:] = gt.extent
        r = ob.OracleRenderer(16, 16)
        r.load_envmap(scenes.HDR)
        r.set_volume(gd, emission=gt, majorant_emission=float(temp.max()))
    else:
        import volren_amd
        r = volren_amd.Renderer(16, 16)
        r.load_envmap(scenes.HDR)
        r.set_volume_dense(dens, commit=False)
        r.set_volume_dense(temp, name="temperature", commit=True)
    r.density_scale = 50.0
    return r


def _ragged(is_oracle, nbc=(5, 3, 7)):
    """the brick crop of tests/test_gpu_lookups.py test_ragged_brick_counts"""
    import encoder_ref
    a = scenes.crop_bricks(encoder_ref.encode_arrays(scenes.synthetic_density(64)), nbc)
    if is_oracle:
        from oracle import binding as ob
        g = ob.Grid()
        g.set(a["transform"], a["n_bricks"], a["min_maj"], a["brick_counter"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"])
        r = ob.OracleRenderer(16, 16)
        r.load_envmap(scenes.HDR)
        r.set_volume(g)
    else:
        import volren_amd
        r = volren_amd.Renderer(16, 16)
        r.load_envmap(scenes.HDR)
        r.set_volume_brick(a["transform"], a["n_bricks"], a["min_maj"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"], commit=True)
    r.density_scale = 40.0
    return r


def segment_scene(name, is_oracle):
    """the scene `name` of SEGMENT_SCENES on the oracle renderer or on the product's, configured identically"""
    s = SEGMENT_SCENES[name]
    if s["base"] == "emission40":
        r = _emission40(is_oracle)
    elif s["base"] == "ragged":
        r = _ragged(is_oracle)
    else:
        r = scenes.oracle_scene(s["base"], 16, 16) if is_oracle else scenes.hip_scene(s["base"], 16, 16)
    if "density_scale" in s:
        r.density_scale = s["density_scale"]
    if "integrator" in s:
        r.integrator = s["integrator"]
    if not is_oracle:
        if "layout" in s:
            r.majorant_layout = s["layout"]
        if "float_atlas" in s:
            r.tf_float_atlas = s["float_atlas"]
    return r


def host_flags(name):
    s = SEGMENT_SCENES[name]
    return (HS_MAJ_BLOCKED if s.get("layout") == 1 else 0) | (HS_NO_FLOAT_ATLAS if s.get("float_atlas") == 0 else 0) | (HS_PAIR if s["base"].startswith("c5") else 0)


def index_extent(o):
    """the density grid's extent in voxels, (x, y, z)"""
    return tuple(o.density.extent) if o.density.dense is not None else tuple(8 * n for n in o.density.n_bricks)


_CASES = {}


def segment_case(name):
    """The oracle's side of one scene, computed once per process and shared: (oracle renderer, compared = {set: (items, want)}, bounded = {set: (items, want)}).
    compared: the sets the budget condition covers; bounded: the scene's over_budget classes and the `stall` set.  Nothing here calls an unbounded function."""
    if name not in _CASES:
        s = SEGMENT_SCENES[name]
        o = segment_scene(name, True)
        p = o.params()
        compared, bounded = {}, {}
        for sn, items in segment_sets(p, index_extent(o), thin=s.get("thin", 1)).items():
            (bounded if sn in s.get("over_budget", ()) else compared)[sn] = (items, o.path_probe(SEGMENT, items))
        st = stall_items(p)
        bounded["stall"] = (st, o.path_probe(SEGMENT, st))
        _CASES[name] = (o, compared, bounded)
    return _CASES[name]


def check_segments(name, probe, form):
    """`probe(kind, form, items)` against segment_case(name): the compared sets in full, the bounded ones where the oracle finished (an item it did not finish only
    has to come back, with a status).  Returns the results per set."""
    o, compared, bounded = segment_case(name)
    results = {}
    for group, full in ((compared, True), (bounded, False)):
        for sn, (items, want) in group.items():
            got = probe(SEGMENT, form, items)
            results[sn] = got
            assert got.shape == (len(items), 14) and (got[:, STATUS_WORD] <= 3).all(), (name, sn, form)
            done = want[:, STATUS_WORD] != 3                      # (the compared sets: nearly all, by the budget condition; the others are held to "came back")
            assert same(SEGMENT, got[done, :SEGMENT_COMPARED], want[done]), "scene %s set %s form %d: %s" % (
                name, sn, form, first_difference(SEGMENT, items[done], got[done, :SEGMENT_COMPARED], want[done]))
    return results
