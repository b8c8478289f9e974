"""CPU: every scene-data lookup of the device code (volren_amd/csrc/vr_probe.h: the accessors of vr_trace.h in the compile-time forms the kernels instantiate),
compiled for the host by tests/hostkernel/probe_host.cpp on tables built as the product builds them (host_scene.h), against the oracle's batch lookups --
bit for bit, over whole tables and their edges, not only along the rays a frame casts.  tests/test_gpu_lookups.py runs the same probes on the device."""
import subprocess
import sys

import numpy as np
import pytest

import hp_binding as hp
import lookup_cases as lc
import scenes
from oracle import binding as ob


def _check(scene, o, what, form, items, orc_what=None):
    got = scene.probe(what, form, items)
    want = o.probe(what if orc_what is None else orc_what, items)
    assert lc.same(got, want), "probe %d form %d: %s" % (what, form, lc.first_difference(items, got, want))


def _maj_form(tf, dense, majb, clean=False):
    return (1 if tf else 0) + 2 * dense + 6 * majb + (18 if clean else 0)


def _emission_scene(n=40, other_layout=False):
    import encoder_ref
    dens = scenes.synthetic_density(n)
    temp = np.clip(dens * 0.2 + 0.1 * scenes.synthetic_density(n, seed=99), 0, None).astype(np.float32)
    if other_layout:
        temp = np.concatenate([temp, temp[:, :, :32]], 2)              # 72 voxels in x: 16 x 8 x 8 bricks against the density grid's 8 x 8 x 8
    gd, gt = encoder_ref.encode(dens), encoder_ref.encode(temp)
    o = ob.OracleRenderer(16, 16)
    o.load_envmap(scenes.HDR)
    o.set_volume(gd, emission=gt, majorant_emission=gt.min_maj[1])
    o.density_scale = 60.0
    return o


def _grid_probes(o, s, lut, blocked):
    """voxel, trilinear and majorant probes of one scene in every form it can serve; returns the forms that ran"""
    dense = o.density.dense is not None
    ext = tuple(o.density.extent) if dense else tuple(8 * n for n in o.density.n_bricks)
    ran = []
    for d in ((1, 2) if dense else (0, 2)):
        _check(s, o, lc.VOXEL, d, lc.voxel_box(ext))
        ran.append(("voxel", d, 0))
        for f32 in ((0, 1) if s.float_atlas else (0,)):
            _check(s, o, lc.TRILINEAR, d + 6 * f32, lc.trilinear_points(ext, n=1 << 13))
            ran.append(("trilinear", d, f32))
    if o.emission is not None:
        eext = tuple(8 * n for n in o.emission.n_bricks)
        _check(s, o, lc.VOXEL, 2, lc.voxel_box(eext, grid=1))
        _check(s, o, lc.TRILINEAR, 2, lc.trilinear_points(eext, grid=1, n=1 << 12))
        if s.paired:
            _check(s, o, lc.VOXEL, 3, lc.voxel_box(ext))                          # PAIR = 1: the density half of the paired atlas
            _check(s, o, lc.VOXEL, 6, lc.voxel_box(eext, grid=1))                 # PAIR = 2: the emission half
            _check(s, o, lc.TRILINEAR, 3, lc.trilinear_points(ext, n=1 << 13))
            ran += [("voxel", 0, 1), ("voxel", 0, 2), ("trilinear-pair", 0, 1)]
    nb = o.density.n_bricks
    for d, m in (((1, 0),) if dense else ((0, 1 if blocked else 0),)) + ((2, 2),):
        if m != 2 and bool(m) != blocked:
            continue
        _check(s, o, lc.MAJORANT, _maj_form(lut, d, m), lc.majorant_cells(nb))
        ran.append(("majorant", d, m))
        if d != 2:
            _check(s, o, lc.MAJORANT, _maj_form(lut, d, m, clean=True), lc.majorant_cells(nb, clean=True))
            ran.append(("majorant-clean", d, m))
    return ran


def _opaque_lut():
    rs = np.random.RandomState(5)
    lut = rs.uniform(0, 1, (16, 4)).astype(np.float32)
    lut[:, 3] = np.sort(lut[:, 3])[::-1]
    return lut


@pytest.mark.parametrize("lut", [None, "file", "opaque"])
@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -16, 2.0 ** 24])
def test_grid_lookups_smoke_brick(lut, blocked, scale):
    """smoke.brick: every voxel of the padded extent plus a ring of 2, every majorant cell of every level plus the rings outside the real extent and the padded
    box, trilinear points on and off the borders -- with and without a LUT (one whose "outside" majorant is not 0 among them), both table layouts, three scales."""
    o = scenes.oracle_scene("c2", 16, 16)
    if lut == "file":
        o.load_transferfunc(scenes.LUT)
    elif lut == "opaque":
        o.set_transferfunc(_opaque_lut())
        o.tf_window_left, o.tf_window_width = -0.2, 0.9
    o.density_scale = scale
    s = hp.Scene(o, hp.MAJ_BLOCKED if blocked else 0)
    assert s.float_atlas == (lut is not None)
    ran = _grid_probes(o, s, lut is not None, blocked)
    assert ("majorant", 0, 1 if blocked else 0) in ran and ("majorant", 2, 2) in ran
    if lut is not None:
        _check(s, o, lc.TF, 0, lc.tf_densities())
    else:
        with pytest.raises(hp.Refused):
            s.probe(lc.TF, 0, lc.tf_densities(8))
    s.close()


@pytest.mark.parametrize("nbc", [(5, 3, 7), (1, 2, 1), (8, 7, 3)])
def test_grid_lookups_ragged_brick_counts(nbc):
    import encoder_ref
    a = scenes.crop_bricks(encoder_ref.encode_arrays(scenes.synthetic_density(64)), nbc)
    g = ob.Grid()
    g.set(a["transform"], a["n_bricks"], a["min_maj"], a["brick_counter"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"])
    o = ob.OracleRenderer(16, 16)
    o.load_envmap(scenes.HDR)
    o.set_volume(g)
    for blocked in (False, True):
        s = hp.Scene(o, hp.MAJ_BLOCKED if blocked else 0)
        _grid_probes(o, s, False, blocked)
        s.close()


def test_grid_lookups_dense_fp16_ragged_extent():
    """a dense fp16 grid whose extents are no multiples of 4 (the blocked layout's last blocks are partial): the voxel array itself is the reference"""
    import encoder_ref
    dens = scenes.synthetic_density(44)[:37, :30, :43].copy()
    o = ob.OracleRenderer(16, 16)
    o.load_envmap(scenes.HDR)
    o.set_volume(encoder_ref.encode_dense_fp16(dens))
    s = hp.Scene(o)
    ran = _grid_probes(o, s, False, False)
    assert ("voxel", 1, 0) in ran and ("majorant-clean", 1, 0) in ran
    items = lc.voxel_box((43, 30, 37), ring=0)
    got = s.probe(lc.VOXEL, 1, items)[:, 0].reshape(37, 30, 43)
    assert lc.same(got, dens.astype(np.float16).astype(np.float32))
    with pytest.raises(hp.Refused):
        s.probe(lc.VOXEL, 0, items)                                  # DENSE = 0 on a dense grid is refused, not guessed
    s.close()


@pytest.mark.parametrize("other_layout", [False, True])
@pytest.mark.parametrize("lut", [False, True])
def test_grid_lookups_emission_scene(other_layout, lut):
    """density + emission grid: with the same brick layout the harness pairs the atlases (its own writer of vr_scene.h's layout) and the PAIR = 1, 2 forms read them;
    with another layout there is no paired atlas and those forms are refused"""
    o = _emission_scene(other_layout=other_layout)
    if lut:
        o.load_transferfunc(scenes.LUT)
    for blocked in (False, True):
        s = hp.Scene(o, hp.PAIR | (hp.MAJ_BLOCKED if blocked else 0))
        assert s.paired == (not other_layout)
        ran = _grid_probes(o, s, lut, blocked)
        assert (("voxel", 0, 2) in ran) == (not other_layout)
        if other_layout:
            with pytest.raises(hp.Refused):
                s.probe(lc.VOXEL, 3, lc.voxel_box((8, 8, 8)))
        s.close()


ENV_MAPS = {
    "hdr": lambda: ob.load_hdr(scenes.HDR),
    "rgbe1x1": lambda: lc.rgbe_map(1, 1), "rgbe2x1": lambda: lc.rgbe_map(2, 1), "rgbe3x2": lambda: lc.rgbe_map(3, 2), "rgbe33x17": lambda: lc.rgbe_map(33, 17),
    "float3x2": lambda: lc.nudged(lc.rgbe_map(3, 2)), "float33x17": lambda: lc.nudged(lc.rgbe_map(33, 17)),
    "rgbe511x257": lambda: lc.rgbe_map(511, 257), "rgbe4100x3": lambda: lc.rgbe_map(4100, 3),
    "dark_patch": lc.dark_patch_map, "black": lambda: np.zeros((4, 8, 3), np.float32), "one_lit": lc.one_lit_map,
}


@pytest.mark.parametrize("name", sorted(ENV_MAPS))
def test_environment_lookups(name):
    """Importance: every texel of every level.  Texel: every centre and edge, the special coordinates, 2^18 random points, float and compact form.  Sky directions.
    Light samples: one targeted draw per base-level texel, the thresholds of the three coarsest levels +- one ulp, a 1024^2 lattice -- by the record-by-record
    sampler and, where the warp table passed the division check, by the block-load / div_core one."""
    env = ENV_MAPS[name]()
    o = scenes.oracle_scene("c2", 16, 16)
    o.set_envmap(env)
    o.env_strength = 1.7
    o.set_env_rot(33.0)
    s = hp.Scene(o)
    assert s.compact == (name.startswith("rgbe") or name in ("hdr", "black", "one_lit")), name
    assert s.div_safe == (name != "dark_patch")
    h, w = env.shape[:2]
    _check(s, o, lc.IMPORTANCE, 0, lc.importance_all())
    avg = o.probe(lc.IMPORTANCE, np.array([[0, 0, 9, 0]], np.int32))
    for form in (1, 2):
        assert lc.same(s.probe(lc.IMPORTANCE, form, np.zeros((1, 4), np.int32)), avg)
    tex = lc.texel_points(w, h, n_random=1 << 18)
    _check(s, o, lc.TEXEL, 0, tex)
    if s.compact:
        _check(s, o, lc.TEXEL, 1, tex)
    else:
        with pytest.raises(hp.Refused):
            s.probe(lc.TEXEL, 1, tex[:4])
    _check(s, o, lc.SKY, 0, lc.sky_directions())
    forms = (0, 1) if s.div_safe else (1,)
    if not s.div_safe:
        with pytest.raises(hp.Refused):
            s.probe(lc.LIGHT, 0, lc.light_lattice(4))
    sets = [lc.light_thresholds(o.impmap), lc.light_lattice(1024)]
    base = lc._levels(o.impmap)[0]
    if (base > 0).any():                                  # (an all-black map -- "black", and the 1x1 map, whose one texel is black -- has no lit texel: sets (b), (c) only)
        items, tx, ty = lc.light_targeted(o.impmap)
        sets.append(items)
        _, hit = o.probe(lc.LIGHT, items, texel=True)
        lit = int((base > 0).sum())
        own = (hit[:, 0] == tx) & (hit[:, 1] == ty) & (base[ty, tx] > 0)
        share = own.sum() / lit
        # at most 1 % of the lit texels may be missed by their own draw as the oracle resolves it; the dark-patch map (texels of 1e-30 that no float32
        # draw reaches) is exempt and held to the oracle's own share instead: 253 952 of 262 144 = 0.96875
        assert share >= (0.96875 if name == "dark_patch" else 0.99), "targeted draws reach %.4f of the %d lit texels" % (share, lit)
    for items in sets:
        for form in forms:
            _check(s, o, lc.LIGHT, form, items)
    s.close()


def test_rgbe_packer():
    """env_pack.h: every texel of the HDR fixture round-trips through pack and env_texture's decode; a black texel packs to 0; each of these alone makes a map
    keep its float form: a negative component, -0.0, inf, NaN, a mantissa that needs 9 bits, an exponent below e = 10 or above 255."""
    env = np.ascontiguousarray(ob.load_hdr(scenes.HDR), np.float32).reshape(-1, 3)
    q = hp.pack_map(env)
    assert q is not None
    assert lc.same(hp.unpack_texels(q), env)
    assert hp.pack_texel([0.0, 0.0, 0.0]) == 0
    ok = np.array([[1.0, 0.5, 0.25]], np.float32)
    assert hp.pack_texel(ok[0]) == (128 | (64 << 8) | (32 << 16) | (129 << 24))
    assert lc.same(hp.unpack_texels([hp.pack_texel(ok[0])]), ok)
    bad = {
        "negative": [1.0, -0.5, 0.25], "minus zero": [1.0, -0.0, 0.25], "inf": [np.inf, 0.5, 0.25], "nan": [1.0, np.nan, 0.25],
        "9-bit mantissa": [1.0, 0.5 + 2.0 ** -9, 0.25], "9 bits below the maximum": [255.0, 0.5, 0.0],
        "exponent below 10": [2.0 ** -127, 0.0, 0.0], "exponent above 255": [2.0 ** 127 * 1.5, 0.0, 0.0],
    }
    assert hp.pack_texel([2.0 ** -126 * 128, 0.0, 0.0]) == (128 | (10 << 24))             # e = 10: the smallest scale kept
    assert hp.pack_texel([255.0 * 2.0 ** 119, 0.0, 0.0]) == (255 | (255 << 24))             # e = 255: the largest
    for why, t in bad.items():
        assert hp.pack_texel(t) is None, why
        m = np.tile(ok, (5, 1))
        m[3] = t
        assert hp.pack_map(m) is None, why
        o = scenes.oracle_scene("c2", 16, 16)
        o.set_envmap(m.reshape(1, 5, 3))
        s = hp.Scene(o)
        assert not s.compact, why
        s.close()


def test_probe_harness_under_ubsan():
    """The probe harness under UndefinedBehaviorSanitizer (GPU sanitizers are not available on the pool: CPU build only): the PAIR = 1, 2 and MAJB = 0, 1 forms,
    the compact decode, the seam branch and both samplers -- none of which the lane-code harness runs."""
    so = hp.build(sanitize=True)
    code = (
        "import sys; sys.path[:0]=[%r,%r]\n"
        "import ctypes as C, numpy as np, hp_binding as hp, lookup_cases as lc, test_lookups_host as t\n"
        "hp.build = lambda sanitize=False: %r\n"
        "for blocked in (False, True):\n"
        "    o = t._emission_scene(n=24); o.load_transferfunc(t.scenes.LUT)\n"
        "    s = hp.Scene(o, hp.PAIR | (hp.MAJ_BLOCKED if blocked else 0)); assert s.paired\n"
        "    ran = t._grid_probes(o, s, True, blocked); assert ('voxel', 0, 2) in ran; s.close()\n"
        "o = t.scenes.oracle_scene('c2', 16, 16); o.set_envmap(lc.rgbe_map(3, 2)); s = hp.Scene(o); assert s.compact\n"
        "for what, items in ((lc.TEXEL, lc.texel_points(3, 2, 4096)), (lc.SKY, lc.sky_directions(4096)), (lc.LIGHT, lc.light_lattice(64))):\n"
        "    for form in ((0, 1) if what != lc.SKY else (0,)): t._check(s, o, what, form, items)\n"
        "print('ok')\n"
    ) % (scenes.ROOT, scenes.ROOT + "/tests", so)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


@pytest.mark.parametrize("kind,extent", scenes.HOSTILE_CASES + (("nan", (65, 9, 8)), ("nan", (129, 8, 8)), ("minus_zero", (65, 9, 8)), ("minus_zero", (3, 70, 1))),
                         ids=["%s-%dx%dx%d" % ((k,) + e) for k, e in scenes.HOSTILE_CASES + (("nan", (65, 9, 8)), ("nan", (129, 8, 8)), ("minus_zero", (65, 9, 8)), ("minus_zero", (3, 70, 1)))])
def test_host_encoder_equals_reference_on_hostile_inputs(kind, extent, tmp_path):
    """The host encoder (vr_write_brick_from_dense, no device needed) against tests/encoder_ref.py, every array bit for bit, on the inputs that
    tests/test_gpu_lookups.py::test_device_encoder_on_hostile_inputs gives the device encoder -- and on NaN voxels, which all three leave out of a brick's range
    and quantise to a defined 0, and on -0.0 voxels, where all three make a zero range bound +0.0."""
    import encoder_ref
    import volren_amd
    lib = volren_amd.load()
    dens = scenes.hostile_dense(kind, extent)
    nz, ny, nx = dens.shape
    path = str(tmp_path / "h.brick")
    assert lib.vr_write_brick_from_dense(dens.ctypes.data, nx, ny, nz, None, path.encode()) == 0, lib.vr_last_error()
    g = ob.Grid.from_file(path)
    with np.errstate(all="ignore"):
        ref = encoder_ref.encode_arrays(dens)
    assert tuple(g.n_bricks) == tuple(ref["n_bricks"]) and g.brick_counter == ref["brick_counter"] and tuple(g.atlas_dim) == tuple(ref["atlas_dim"])
    assert np.array_equal(g.indirection, ref["indirection"]) and np.array_equal(g.range, ref["rng"])
    assert np.array_equal(g.atlas, ref["atlas"])
    for (d1, a1), (d2, a2) in zip(g.mips, ref["mips"]):
        assert tuple(d1) == tuple(d2) and np.array_equal(a1, a2)


def test_probes_see_one_changed_table_entry():
    """The comparisons above are only worth what they can see: one byte of the harness's paired atlas flipped, one majorant cell zeroed, the top-level warp
    threshold nudged by one ulp -- each in the harness's OWN arrays (hp.Scene.table), nothing of the product -- must make the matching probe differ from the oracle."""
    o = _emission_scene(n=24)
    s = hp.Scene(o, hp.PAIR)
    assert s.paired
    ext = tuple(8 * n for n in o.density.n_bricks)
    vox, mj = lc.voxel_box(ext), lc.majorant_cells(o.density.n_bricks)
    assert lc.same(s.probe(lc.VOXEL, 3, vox), o.probe(lc.VOXEL, vox)) and lc.same(s.probe(lc.MAJORANT, 0, mj), o.probe(lc.MAJORANT, mj))
    atlas = s.table(0, np.uint8)
    rdiff = atlas.view(np.float32).reshape(-1, 320)[:, 1]                 # the density range difference at the head of each brick's first line
    b = int(np.nonzero(rdiff != 0)[0][0])
    atlas[b * 1280 + 16 + 2 * 5] ^= 1                                     # density voxel 5 of that brick
    assert not lc.same(s.probe(lc.VOXEL, 3, vox), o.probe(lc.VOXEL, vox))
    assert lc.same(s.probe(lc.VOXEL, 0, vox), o.probe(lc.VOXEL, vox))     # (the grid's own atlas is untouched)
    m16 = s.table(3, np.uint16)
    m16[int(np.nonzero(m16)[0][0])] = 0
    assert not lc.same(s.probe(lc.MAJORANT, 0, mj), o.probe(lc.MAJORANT, mj))
    s.close()
    o = scenes.oracle_scene("c2", 16, 16)
    s = hp.Scene(o)
    items = lc.light_thresholds(o.impmap)
    assert lc.same(s.probe(lc.LIGHT, 1, items), o.probe(lc.LIGHT, items))
    cdf = s.table(1, np.float32)
    cdf[0] = np.nextafter(cdf[0], np.float32(2))                          # level 0's d (an odd number of levels: its record sits alone in block 0)
    assert not lc.same(s.probe(lc.LIGHT, 1, items), o.probe(lc.LIGHT, items))
    s.close()
