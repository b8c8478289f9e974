"""Scene set-ups shared by the tests, bench.py and smoke(): the BASELINE.json configs on the oracle renderer and on
the HIP renderer, configured identically."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "fixtures")
SMOKE = os.path.join(FIX, "smoke.brick")
HDR = os.path.join(FIX, "table_mountain_2_puresky_1k.hdr")
LUT = os.path.join(FIX, "lut.txt")

# name -> settings.  c1/c2/c3 are BASELINE.json configs[0..2]; "readme" is README.md:72-73 of the reference.
CONFIGS = {
    "c1": dict(bounces=4, cam_fov=40.0),
    "c2": dict(bounces=100, cam_fov=40.0),
    "c3": dict(bounces=100, cam_fov=40.0, lut=True),
    "readme": dict(bounces=128, cam_fov=40.0, albedo=0.8, phase=0.3, density=100.0, env_strength=3.0, env_rot=270.0,
                   exposure=3.0, gamma=2.0),
}


def synthetic_dense_fp16(n=512, seed=1234):
    """BASELINE configs[3] generator: deterministic smoke-like n^3 field (sum of Gaussian blobs on a coarse lattice,
    tricubically upsampled, ~25 % non-zero, max 5.0) as float16 [z][y][x]."""
    from scipy import ndimage
    coarse = max(32, n // 4)
    f = synthetic_density(coarse, seed=seed, blobs=64).astype(np.float32)
    if coarse != n:
        f = ndimage.zoom(f, n / coarse, order=1, mode="nearest", prefilter=False)[:n, :n, :n]
    f = np.clip(f, 0, None)
    return np.ascontiguousarray(f * np.float32(5.0 / max(float(f.max()), 1e-6))).astype(np.float16)


_DENSE_CACHE = {}


def configure_dense(r, is_oracle, n=512):
    """BASELINE configs[3] ('c4'): synthetic n^3 dense fp16 grid + the README.md:72-73 rendering parameters."""
    if n not in _DENSE_CACHE:
        _DENSE_CACHE[n] = synthetic_dense_fp16(n)
    vox = _DENSE_CACHE[n]
    if is_oracle:
        import encoder_ref
        r.set_volume(encoder_ref.encode_dense_fp16(vox))
    else:
        r.set_volume_dense_f16(vox)
    r.load_envmap(HDR)
    cfg = CONFIGS["readme"]
    r.bounces, r.cam_fov = 128, 40.0
    r.albedo = (cfg["albedo"],) * 3
    r.phase = cfg["phase"]
    r.density_scale = cfg["density"]
    r.env_strength = cfg["env_strength"]
    if is_oracle:
        r.set_env_rot(cfg["env_rot"])
    else:
        r.env_rot = cfg["env_rot"]
    r.tonemap_exposure, r.tonemap_gamma = cfg["exposure"], cfg["gamma"]
    return r


def synthetic_sparse_pair(n=512, seed=4321):
    """BASELINE configs[4] generator: cloud-like sparse density (~15 % of the voxels non-zero, max 5.0) and a temperature
    grid correlated with it, float32 [z][y][x]."""
    from scipy import ndimage
    coarse = max(32, n // 4)
    base = synthetic_density(coarse, seed=seed, blobs=48).astype(np.float32)
    det = synthetic_density(coarse, seed=seed + 1, blobs=96).astype(np.float32)
    dens = np.maximum(base - np.quantile(base, 0.85 - 0.25) * 0 - 0.35 * base.max(), 0)     # keep the cores of the blobs
    temp = np.maximum(dens * 0.6 + 0.2 * det * (dens > 0), 0)
    if coarse != n:
        z = n / coarse
        dens = ndimage.zoom(dens, z, order=1, mode="nearest", prefilter=False)[:n, :n, :n]
        temp = ndimage.zoom(temp, z, order=1, mode="nearest", prefilter=False)[:n, :n, :n]
    dens = np.ascontiguousarray(np.clip(dens, 0, None) * np.float32(5.0 / max(float(dens.max()), 1e-6)), np.float32)
    temp = np.ascontiguousarray(np.clip(temp, 0, None) * np.float32(1.0 / max(float(temp.max()), 1e-6)), np.float32)
    return dens, temp


def configure_sparse(r, is_oracle, n=512):
    """BASELINE configs[4] ('c5'): synthetic sparse brick grid + temperature grid, emission on (common.glsl:324-328,489)."""
    key = ("c5", n)
    if key not in _DENSE_CACHE:
        _DENSE_CACHE[key] = synthetic_sparse_pair(n)
    dens, temp = _DENSE_CACHE[key]
    if is_oracle:
        import encoder_ref
        gd, gt = encoder_ref.encode(dens), encoder_ref.encode(temp)
        for g in (gd, gt):                          # an in-memory dense grid keeps its voxel extent (see grid_to_device)
            g.extent = (n, n, n)
            g.c.extent[:] = g.extent
        r.set_volume(gd, emission=gt, majorant_emission=float(temp.max()))
    else:
        r.set_volume_dense(dens, commit=False)
        r.set_volume_dense(temp, name="temperature", commit=True)
    r.load_envmap(HDR)
    r.bounces, r.cam_fov = 128, 40.0
    r.albedo = (0.9, 0.9, 0.9)
    r.phase = 0.3
    r.density_scale = 100.0
    r.emission_scale = 100.0
    return r


def configure(r, name, is_oracle):
    if name.startswith("c5cloud"):
        return configure_cloud(r, is_oracle, int(name[8:]) if len(name) > 8 else 1024)
    if name.startswith("c5full"):
        return configure_sparse_full(r, is_oracle, int(name[7:]) if len(name) > 7 else 1024)
    if name.startswith("c5"):
        return configure_sparse(r, is_oracle, int(name[3:]) if len(name) > 3 else 512)
    if name.startswith("c4"):
        return configure_dense(r, is_oracle, int(name[3:]) if len(name) > 3 else 512)
    """Apply a config in the reference's command-line order (paths first, then overrides: main.cpp:360-435)."""
    cfg = CONFIGS[name]
    r.load_volume(SMOKE)
    r.load_envmap(HDR)
    if cfg.get("lut"):
        r.load_transferfunc(LUT)
    r.bounces = cfg["bounces"]
    r.cam_fov = cfg["cam_fov"]
    if "albedo" in cfg:
        r.albedo = (cfg["albedo"],) * 3
    if "phase" in cfg:
        r.phase = cfg["phase"]
    if "density" in cfg:
        r.density_scale = cfg["density"]
    if "env_strength" in cfg:
        r.env_strength = cfg["env_strength"]
    if "env_rot" in cfg:
        if is_oracle:
            r.set_env_rot(cfg["env_rot"])
        else:
            r.env_rot = cfg["env_rot"]
    if "exposure" in cfg:
        r.tonemap_exposure = cfg["exposure"]
        r.tonemap_gamma = cfg["gamma"]
    return r


def configure_r5(r, name, is_oracle):
    """Round 5's extra views of smoke.brick (tests/golden/host_rows.py R5_SCENES): config c2 plus another camera / a rotated environment / a cropped
    volume, applied through the renderer's setters in the reference's command-line order (src/main.cpp:360-435)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import host_rows as hr
    s = hr.R5_SCENES[name]
    configure(r, "c2", is_oracle)
    r.cam_pos, r.cam_dir, r.cam_up, r.cam_fov = s["cam_pos"], tuple(float(x) for x in hr.scene_dir(s)), s["cam_up"], s["cam_fov"]
    if "env_rot" in s:
        if is_oracle:
            r.set_env_rot(s["env_rot"])
        else:
            r.env_rot = s["env_rot"]
        r.env_strength = s["env_strength"]
    if "density" in s:
        r.density_scale = s["density"]
    if "vol_crop_min" in s:
        r.vol_clip_min, r.vol_clip_max = s["vol_crop_min"], s["vol_crop_max"]
    return r


def oracle_scene(name, w, h):
    from oracle import binding as ob
    return configure(ob.OracleRenderer(w, h), name, True)


def hip_scene(name, w, h, device=0):
    import volren_amd
    return configure(volren_amd.Renderer(w, h, device=device), name, False)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def synthetic_density(n, seed=1234, blobs=24):
    """Deterministic smoke-like dense field [z][y][x] in [0, 5], ~25 % non-zero (SURVEY 8d, C4 generator, small)."""
    rs = np.random.RandomState(seed)
    z, y, x = np.meshgrid(*(np.linspace(0, 1, n, dtype=np.float32),) * 3, indexing="ij")
    f = np.zeros((n, n, n), np.float32)
    for _ in range(blobs):
        c = rs.uniform(0.2, 0.8, 3).astype(np.float32)
        s = np.float32(rs.uniform(0.05, 0.15))
        a = np.float32(rs.uniform(0.3, 1.0))
        f += a * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    thr = np.quantile(f, 0.75)
    f = np.maximum(f - thr, 0)
    return (f * (5.0 / f.max())).astype(np.float32)


def _range_mips(lo, hi):
    """Three (min of mins, max of maxes) levels over 2x2x2 children, as encoder_ref.encode_arrays builds them."""
    mips = []
    for _ in range(3):
        z, y, x = lo.shape
        z2, y2, x2 = (z + 1) // 2, (y + 1) // 2, (x + 1) // 2
        plo = np.full((z2 * 2, y2 * 2, x2 * 2), np.inf, np.float32)
        phi = np.full((z2 * 2, y2 * 2, x2 * 2), -np.inf, np.float32)
        plo[:z, :y, :x] = lo
        phi[:z, :y, :x] = hi
        lo = plo.reshape(z2, 2, y2, 2, x2, 2).min((1, 3, 5))
        hi = phi.reshape(z2, 2, y2, 2, x2, 2).max((1, 3, 5))
        w = lo.astype(np.float16).view(np.uint16).astype(np.uint32) | (hi.astype(np.float16).view(np.uint16).astype(np.uint32) << 16)
        mips.append(((x2, y2, z2), w.reshape(-1)))
    return mips


def crop_bricks(a, nbc):
    """Centred sub-block nbc = (cx, cy, cz) of an encode_arrays() brick grid: indirection/range cropped (the atlas pointers stay
    valid), range mips rebuilt with the ceil(n / 2) rule (min of mins, max of maxes over the existing children)."""
    nbx, nby, nbz = a["n_bricks"]
    cx, cy, cz = nbc
    ox, oy, oz = (nbx - cx) // 2, (nby - cy) // 2, (nbz - cz) // 2          # centred: the synthetic cloud is densest there
    ind = a["indirection"].reshape(nbz, nby, nbx)[oz:oz + cz, oy:oy + cy, ox:ox + cx].copy()
    rng = a["rng"].reshape(nbz, nby, nbx)[oz:oz + cz, oy:oy + cy, ox:ox + cx].copy()
    lo = (rng & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    hi = (rng >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
    mips = []
    for _ in range(3):
        z, y, x = lo.shape
        z2, y2, x2 = (z + 1) // 2, (y + 1) // 2, (x + 1) // 2
        plo = np.full((z2 * 2, y2 * 2, x2 * 2), np.inf, np.float32)
        phi = np.full((z2 * 2, y2 * 2, x2 * 2), -np.inf, np.float32)
        plo[:z, :y, :x] = lo
        phi[:z, :y, :x] = hi
        lo = plo.reshape(z2, 2, y2, 2, x2, 2).min((1, 3, 5))
        hi = phi.reshape(z2, 2, y2, 2, x2, 2).max((1, 3, 5))
        w = lo.astype(np.float16).view(np.uint16).astype(np.uint32) | (hi.astype(np.float16).view(np.uint16).astype(np.uint32) << 16)
        mips.append(((x2, y2, z2), w.reshape(-1)))
    out = dict(a)
    out.update(n_bricks=(cx, cy, cz), indirection=ind.reshape(-1), rng=rng.reshape(-1), mips=mips)
    return out


_SPARSE_FULL = {}


def sparse_brick_arrays_full(n=1024, chunks=160, seed=777):
    """BASELINE configs[4]'s grid SIZE (n^3 voxels, (n/8)^3 bricks, a few per cent of them allocated) built directly in brick
    form -- the dense n^3 array is never materialised, so the scene takes seconds, not minutes: `chunks` cells of a 64-voxel
    lattice each hold one smooth blob that vanishes 4 voxels inside the cell border (so the +-2-voxel range dilation never
    crosses cells and every cell can be encoded on its own by the numpy reference encoder), everything else is empty.
    Returns (density, temperature) as encode_arrays()-style dicts: the exact input of vr_set_volume_brick / oracle Grid.set."""
    key = (n, chunks, seed)
    if key in _SPARSE_FULL:
        return _SPARSE_FULL[key]
    import encoder_ref
    c = 64
    cells = n // c
    nb = n // 8
    rs = np.random.RandomState(seed)
    # blobs cluster around the centre so that a camera looking at the origin sees overlapping ones
    pick = set()
    while len(pick) < chunks:
        p = tuple(np.clip(np.round(rs.normal(cells / 2 - 0.5, cells / 6, 3)), 0, cells - 1).astype(int))
        pick.add(p)
    zz, yy, xx = np.meshgrid(*(np.arange(c, dtype=np.float32) - (c - 1) / 2,) * 3, indexing="ij")
    r2 = xx * xx + yy * yy + zz * zz
    out = []
    for which in ("density", "temperature"):
        rng_w = np.zeros((nb, nb, nb), np.uint32)
        ind = np.zeros((nb, nb, nb), np.uint32)
        blocks = []
        for (cz, cy, cx) in sorted(pick):
            rr = np.random.RandomState(hash((cz, cy, cx, seed)) & 0x7FFFFFFF)
            sigma = np.float32(rr.uniform(8.0, 13.0))
            amp = np.float32(rr.uniform(1.0, 5.0))
            f = np.exp(-r2 / (2 * sigma * sigma)) - np.float32(np.exp(-28.0 * 28.0 / (2 * sigma * sigma)))
            wob = 1 + np.float32(0.25) * np.sin(xx * np.float32(rr.uniform(0.2, 0.5))) * np.cos(yy * np.float32(rr.uniform(0.2, 0.5)) + zz * np.float32(0.3))
            f = (np.maximum(f, 0) * wob * amp).astype(np.float32)
            if which == "temperature":
                f = (np.clip(f / amp, 0, 1) ** 2 * np.float32(rr.uniform(0.3, 1.0))).astype(np.float32)
            a = encoder_ref.encode_arrays(f)
            lb = c // 8
            l_ind = a["indirection"].reshape(lb, lb, lb)
            l_rng = a["rng"].reshape(lb, lb, lb)
            l_atlas = a["atlas"].reshape(a["atlas_dim"][2], a["atlas_dim"][1], a["atlas_dim"][0])
            rng_w[cz * lb:(cz + 1) * lb, cy * lb:(cy + 1) * lb, cx * lb:(cx + 1) * lb] = l_rng
            lo = (l_rng & 0xFFFF).astype(np.uint16).view(np.float16)
            hi = (l_rng >> 16).astype(np.uint16).view(np.float16)
            for bz, by, bx in zip(*np.nonzero(lo != hi)):
                v = int(l_ind[bz, by, bx])
                px, py, pz = v >> 22, (v >> 12) & 1023, (v >> 2) & 1023
                blocks.append(((cz * lb + bz, cy * lb + by, cx * lb + bx), l_atlas[pz * 8:pz * 8 + 8, py * 8:py * 8 + 8, px * 8:px * 8 + 8]))
        per_layer = nb * nb
        layers = max(1, (len(blocks) + per_layer - 1) // per_layer)
        atlas = np.zeros((layers * 8, nb * 8, nb * 8), np.uint8)
        for k, ((bz, by, bx), blk) in enumerate(blocks):
            px, py, pz = k % nb, (k // nb) % nb, k // per_layer
            ind[bz, by, bx] = (px << 22) | (py << 12) | (pz << 2)
            atlas[pz * 8:pz * 8 + 8, py * 8:py * 8 + 8, px * 8:px * 8 + 8] = blk
        lo_f = (rng_w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
        hi_f = (rng_w >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
        out.append(dict(transform=np.eye(4, dtype=np.float32).reshape(16), n_bricks=(nb, nb, nb), min_maj=(float(lo_f.min()), float(hi_f.max())),
                        brick_counter=len(blocks), indirection=ind.reshape(-1), rng=rng_w.reshape(-1),
                        atlas_dim=(nb * 8, nb * 8, layers * 8), atlas=atlas.reshape(-1), mips=_range_mips(lo_f, hi_f)))
    _SPARSE_FULL[key] = tuple(out)
    return _SPARSE_FULL[key]


_CLOUD = {}
_CLOUD_DENSE = {}


def _half_outward(lo, hi):
    """fp16 range of encoder_ref.encode_arrays, vectorised: minimum rounded down, maximum rounded up."""
    hl = lo.astype(np.float16)
    hl = np.where(hl.astype(np.float32) > lo, np.nextafter(hl, np.float16(-np.inf)), hl)
    hh = hi.astype(np.float16)
    hh = np.where(hh.astype(np.float32) < hi, np.nextafter(hh, np.float16(np.inf)), hh)
    return hl, hh


def _window_minmax(pad, nb):
    """(min, max) over the 12^3 neighbourhood (8^3 brick dilated by 2 voxels) of each of the nb^3 bricks of a padded block [8 nb + 4]^3."""
    lo, hi = pad, pad
    for axis in range(3):
        idx = [slice(None)] * 3
        los, his = [], []
        for b in range(nb):
            idx[axis] = slice(8 * b, 8 * b + 12)
            los.append(lo[tuple(idx)].min(axis=axis, keepdims=True))
            his.append(hi[tuple(idx)].max(axis=axis, keepdims=True))
        lo, hi = np.concatenate(los, axis=axis), np.concatenate(his, axis=axis)
    return lo, hi


def cloud_brick_arrays(n=1024, seed=2026, target=0.15):
    """BASELINE configs[4] as SURVEY 8d specifies it ('c5cloud'): an n^3 sparse brick grid of wdas_cloud-like occupancy -- 10-20 % of its (n/8)^3
    bricks allocated (1024^3: ~300 000 of 2 097 152) -- holding ONE connected cloud: an ellipsoidal body modulated by five octaves of noise
    (amplitude ~ 1 / frequency), thresholded, maximum 5.0, plus a temperature grid correlated with the density (emission).  Built directly in brick
    form, 64^3-voxel blocks at a time (the dense 4 GiB array is never materialised): the field is a sum of separable products of 1-D sinusoids,
    so a block with its 2-voxel halo is one small matrix product, and blocks that the field's Lipschitz bound proves empty are skipped.  The
    encoding rules are encoder_ref.encode_arrays' (dilated fp16 ranges rounded outwards, u8 quantisation), vectorised; test_cloud_generator_*
    checks that on a small n against that encoder.  Returns (density, temperature) dicts: the input of vr_set_volume_brick / oracle Grid.set."""
    key = (n, seed, target)
    if key in _CLOUD:
        return _CLOUD[key]
    rs = np.random.RandomState(seed)
    nb = n // 8
    c = min(64, n)                       # block edge in voxels
    cells = n // c
    lb = c // 8
    # noise: octave o has wavelength n / (3 * 2^o) voxels (>= 21 voxels at n = 1024: smooth at the voxel scale), amplitude 2^-o, 6 terms each
    terms = []
    for o in range(5):
        for _ in range(6):
            w = 2.0 * np.pi * 3.0 * (2 ** o) / n * rs.uniform(0.7, 1.3, 3)
            terms.append((rs.uniform(0.6, 1.0) * 0.5 ** o * rs.choice([-1.0, 1.0]), w, rs.uniform(0, 2 * np.pi, 3)))
    amp = np.array([t[0] for t in terms], np.float32)
    freq = np.array([t[1] for t in terms])
    phase = np.array([t[2] for t in terms])
    axis_pos = np.arange(-2, n + 2, dtype=np.float64)                                   # voxel centres incl. the halo
    S = [np.sin(freq[:, a:a + 1] * axis_pos[None, :] + phase[:, a:a + 1]).astype(np.float32) for a in range(3)]     # [K][n + 4] per axis
    centre = np.array([0.5, 0.46, 0.5]) * n
    radii = np.array([0.40, 0.30, 0.36]) * n
    body = [(((axis_pos - centre[a]) / radii[a]) ** 2).astype(np.float32) for a in range(3)]   # 1 - sum = ellipsoidal body
    noise_gain = np.float32(0.55)
    lipschitz = float(noise_gain * np.sum(np.abs(amp) * np.sqrt((freq ** 2).sum(1))) + 2.0 * np.sqrt(3.0) / radii.min())

    def field(z0, z1, y0, y1, x0, x1):
        """raw field (before the threshold) on voxels [z0, z1) x [y0, y1) x [x0, x1), halo indices allowed (-2 .. n + 1)"""
        zs, ys, xs = slice(z0 + 2, z1 + 2), slice(y0 + 2, y1 + 2), slice(x0 + 2, x1 + 2)
        zy = (S[2][:, zs][:, :, None] * S[1][:, ys][:, None, :]).reshape(len(amp), -1)                   # [K][nz * ny]
        nz_, ny_, nx_ = z1 - z0, y1 - y0, x1 - x0
        noise = (zy.T @ (S[0][:, xs] * amp[:, None])).reshape(nz_, ny_, nx_)
        return (np.float32(1.0) - body[2][zs][:, None, None] - body[1][ys][None, :, None] - body[0][xs][None, None, :]) + noise_gain * noise

    # threshold from the field at the brick centres: `target` of the bricks above it
    cz = np.arange(4, n, 8)
    zyc = (S[2][:, cz + 2][:, :, None] * S[1][:, cz + 2][:, None, :]).reshape(len(amp), -1)
    coarse = (np.float32(1.0) - body[2][cz + 2][:, None, None] - body[1][cz + 2][None, :, None] - body[0][cz + 2][None, None, :]) + \
        noise_gain * (zyc.T @ (S[0][:, cz + 2] * amp[:, None])).reshape(nb, nb, nb)
    thr = np.float32(np.quantile(coarse, 1.0 - target * 0.82))           # the dilated ranges allocate ~20 % more bricks than have their centre inside
    peak = np.float32(max(float(coarse.max()) - float(thr), 1e-3))
    scale = np.float32(5.0) / peak
    # a block can only hold non-zero voxels if some brick centre in or next to it comes within reach of the threshold
    reach = np.float32(lipschitz * (4.0 * np.sqrt(3.0) + 2.0 * np.sqrt(3.0)))
    near = np.pad(coarse > thr - reach, 1, mode="constant")
    out = {}
    state = {}
    for which in ("density", "temperature"):
        state[which] = dict(rng=np.zeros((nb, nb, nb), np.uint32), where=[], blocks=[])
    tw = 2.0 * np.pi * 5.0 / n
    full = (np.zeros((n, n, n), np.float32), np.zeros((n, n, n), np.float32)) if n <= 256 else None      # small grids: the dense voxels too (cloud_dense)
    for bz in range(cells):
        for by in range(cells):
            for bx in range(cells):
                if not near[bz * lb:bz * lb + lb + 2, by * lb:by * lb + lb + 2, bx * lb:bx * lb + lb + 2].any():
                    continue
                z0, y0, x0 = bz * c, by * c, bx * c
                raw = field(z0 - 2, z0 + c + 2, y0 - 2, y0 + c + 2, x0 - 2, x0 + c + 2)
                dens = np.minimum(np.maximum(raw - thr, np.float32(0.0)) * scale, np.float32(5.0))
                # outside the grid the encoder sees zeros (encoder_ref pads with 0)
                for a, o in enumerate((z0, y0, x0)):
                    idx = [slice(None)] * 3
                    if o == 0:
                        idx[a] = slice(0, 2); dens[tuple(idx)] = 0
                    if o + c == n:
                        idx[a] = slice(c + 2, c + 4); dens[tuple(idx)] = 0
                if not dens.any():
                    continue
                # temperature: hot core, cooler towards the rim, modulated along y and x; zero wherever the density is
                zi = np.arange(z0 - 2, z0 + c + 2)[:, None, None]
                yi = np.arange(y0 - 2, y0 + c + 2)[None, :, None]
                xi = np.arange(x0 - 2, x0 + c + 2)[None, None, :]
                mod = (np.float32(0.7) + np.float32(0.3) * np.sin(tw * yi + 0.5).astype(np.float32) * np.cos(tw * xi + tw * 0.7 * zi).astype(np.float32))
                temp = (np.square(dens * np.float32(0.2)) * mod).astype(np.float32)
                if full is not None:
                    full[0][z0:z0 + c, y0:y0 + c, x0:x0 + c] = dens[2:c + 2, 2:c + 2, 2:c + 2]
                    full[1][z0:z0 + c, y0:y0 + c, x0:x0 + c] = temp[2:c + 2, 2:c + 2, 2:c + 2]
                for which, v in (("density", dens), ("temperature", temp)):
                    st = state[which]
                    lo, hi = _window_minmax(v, lb)
                    hl, hh = _half_outward(lo, hi)
                    st["rng"][bz * lb:(bz + 1) * lb, by * lb:(by + 1) * lb, bx * lb:(bx + 1) * lb] = hl.view(np.uint16).astype(np.uint32) | (hh.view(np.uint16).astype(np.uint32) << 16)
                    lo32, hi32 = hl.astype(np.float32), hh.astype(np.float32)
                    alloc = hi32 != lo32
                    if not alloc.any():
                        continue
                    inner = v[2:c + 2, 2:c + 2, 2:c + 2].reshape(lb, 8, lb, 8, lb, 8).transpose(0, 2, 4, 1, 3, 5)      # [bz][by][bx][z][y][x]
                    sel = inner[alloc]                                                                                  # [m][8][8][8]
                    l_, h_ = lo32[alloc][:, None, None, None], hi32[alloc][:, None, None, None]
                    inv = np.float32(255.0) / (h_ - l_)
                    q = np.clip(np.floor((sel - l_) * inv + np.float32(0.5)), 0, 255).astype(np.uint8)
                    lz, ly, lx = np.nonzero(alloc)
                    st["where"].append(np.stack([lz + bz * lb, ly + by * lb, lx + bx * lb], 1))
                    st["blocks"].append(q)
    for which in ("density", "temperature"):
        st = state[which]
        where = np.concatenate(st["where"]) if st["where"] else np.zeros((0, 3), np.int64)
        blocks = np.concatenate(st["blocks"]) if st["blocks"] else np.zeros((0, 8, 8, 8), np.uint8)
        order = np.lexsort((where[:, 2], where[:, 1], where[:, 0]))        # slots in brick order (z, y, x), as the sequential encoder hands them out
        where, blocks = where[order], blocks[order]
        m = len(where)
        per_layer = nb * nb
        layers = max(1, (m + per_layer - 1) // per_layer)
        k = np.arange(m)
        ind = np.zeros((nb, nb, nb), np.uint32)
        ind[where[:, 0], where[:, 1], where[:, 2]] = (((k % nb) << 22) | (((k // nb) % nb) << 12) | ((k // per_layer) << 2)).astype(np.uint32)
        tex = np.zeros((layers * per_layer, 8, 8, 8), np.uint8)
        tex[:m] = blocks
        atlas = tex.reshape(layers, nb, nb, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(layers * 8, nb * 8, nb * 8)
        lo_f = (st["rng"] & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
        hi_f = (st["rng"] >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
        out[which] = dict(transform=np.eye(4, dtype=np.float32).reshape(16), n_bricks=(nb, nb, nb), min_maj=(float(lo_f.min()), float(hi_f.max())),
                          brick_counter=m, indirection=ind.reshape(-1), rng=st["rng"].reshape(-1),
                          atlas_dim=(nb * 8, nb * 8, layers * 8), atlas=np.ascontiguousarray(atlas).reshape(-1), mips=_range_mips(lo_f, hi_f))
    _CLOUD[key] = (out["density"], out["temperature"])
    if full is not None:
        _CLOUD_DENSE[key] = full
    return _CLOUD[key]


def cloud_dense(n, seed=2026, target=0.15):
    """The dense voxels (density, temperature) behind cloud_brick_arrays for a small n: what the generator's check hands to encoder_ref.encode_arrays."""
    cloud_brick_arrays(n, seed, target)
    return _CLOUD_DENSE[(n, seed, target)]


def configure_cloud(r, is_oracle, n=1024):
    """BASELINE configs[4] on the grid of cloud_brick_arrays(): the c5 settings (emission on, albedo 0.9, g 0.3, density x 100, 128 bounces)."""
    ad, at = cloud_brick_arrays(n)
    return _configure_brick_pair(r, is_oracle, ad, at)


def configure_sparse_full(r, is_oracle, n=1024):
    """The c5 settings (configure_sparse) on the brick-form full-size grid of sparse_brick_arrays_full()."""
    ad, at = sparse_brick_arrays_full(n)
    return _configure_brick_pair(r, is_oracle, ad, at)


def _configure_brick_pair(r, is_oracle, ad, at):
    if is_oracle:
        from oracle import binding as ob

        def grid(a):
            g = ob.Grid()
            g.set(a["transform"], a["n_bricks"], a["min_maj"], a["brick_counter"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"])
            return g
        r.set_volume(grid(ad), emission=grid(at), majorant_emission=at["min_maj"][1])
    else:
        r.set_volume_brick(ad["transform"], ad["n_bricks"], ad["min_maj"], ad["indirection"], ad["rng"], ad["atlas_dim"], ad["atlas"], ad["mips"], commit=False)
        r.set_volume_brick(at["transform"], at["n_bricks"], at["min_maj"], at["indirection"], at["rng"], at["atlas_dim"], at["atlas"], at["mips"], name="temperature", commit=True)
    r.load_envmap(HDR)
    r.bounces, r.cam_fov = 128, 40.0
    r.albedo = (0.9, 0.9, 0.9)
    r.phase = 0.3
    r.density_scale = 100.0
    r.emission_scale = 100.0
    return r


# ---- hostile inputs of the dense -> brick encoders (tests/test_gpu_lookups.py) -------------------------------------------------------------------
HOSTILE_EXTENTS = ((1, 1, 1), (3, 70, 1), (65, 9, 8), (129, 8, 8))       # (nx, ny, nz); 129 x 8 x 8: the bricks from x = 136 on lie fully outside (x0 >= nx)
HOSTILE_CASES = tuple([("random", e) for e in HOSTILE_EXTENTS] +
                      [(k, (65, 9, 8)) for k in ("constant", "negative", "above_half_max", "1e-7", "1e-9", "denormal", "spikes", "ties", "inf")] +
                      [("constant", (1, 1, 1)), ("negative", (3, 70, 1)), ("spikes", (129, 8, 8)), ("inf", (129, 8, 8))])


def hostile_dense(kind, extent, seed=2027):
    """A dense float32 grid [z][y][x] of extent (nx, ny, nz) that is hard on a dense -> brick encoder; fixed seed.  kinds: random (uniform 0..5), constant,
    negative (-3..1), above_half_max (values beyond fp16's 65504: the range maximum rounds up to inf), 1e-7 / 1e-9 (ranges at and below fp16's smallest
    denormal 6e-8), denormal (float32 denormals), spikes (zero but for a few isolated voxels), ties (values whose quantisation lands exactly on .5),
    inf (+inf voxels among finite ones), minus_zero (-0.0 among the zeros), nan (NaN voxels among finite ones, no 12^3 window of NaN only)."""
    nx, ny, nz = extent
    rs = np.random.RandomState(seed + 131 * nx + 17 * ny + nz + sum(map(ord, kind)))
    u = rs.uniform(0, 1, (nz, ny, nx)).astype(np.float32)
    if kind == "random":
        d = u * np.float32(5)
    elif kind == "constant":
        d = np.full((nz, ny, nx), 2.5, np.float32)
    elif kind == "negative":
        d = u * np.float32(4) - np.float32(3)
    elif kind == "above_half_max":
        d = u * np.float32(1e5)
    elif kind in ("1e-7", "1e-9"):
        d = u * np.float32(float(kind))
    elif kind == "denormal":
        d = (rs.randint(0, 1 << 22, (nz, ny, nx)).astype(np.uint32)).view(np.float32).copy()
    elif kind == "spikes":
        d = np.where(u > 0.985, u * np.float32(40), np.float32(0)).astype(np.float32)
        d.flat[0] = 7.0
    elif kind == "ties":
        d = ((rs.randint(0, 255, (nz, ny, nx)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 / 255.0)).astype(np.float32)
        d.flat[0], d.flat[-1] = 0.0, 2.0                       # a [0, 2] range where nothing is dilated away: (v - lo) * 255 / 2 = k + .5
    elif kind == "inf":
        d = u * np.float32(5)
        d[u > 0.97] = np.inf
    elif kind == "minus_zero":
        d = np.where(u > 0.5, u, np.float32(0)).astype(np.float32)
        d[u < 0.25] = -0.0
    elif kind == "nan":
        d = u * np.float32(5)
        d[u > 0.97] = np.nan
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(d, np.float32)
