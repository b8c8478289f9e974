"""GPU: every scene-data lookup on the device against the oracle, bit for bit -- Renderer.probe (include/volren_amd.h vr_probe) runs the accessors of vr_trace.h
in the compile-time forms the kernels instantiate, on the tables the device's builder kernels made (importance pyramid, warp table, device brick encoder, paired
and decoded float atlas, majorant tables), over WHOLE tables and their edges instead of along the rays of a frame.  tests/test_lookups_host.py runs the same
probes, from the same header, on the CPU."""
import numpy as np
import pytest

import lookup_cases as lc
import scenes

pytestmark = pytest.mark.gpu


def _check(r, o, what, form, items):
    got = r.probe(what, form, items)
    want = o.probe(what, items)
    assert lc.same(got, want), "probe %d form %d: %s" % (what, form, lc.first_difference(items, got, want))


def _maj_form(tf, dense, majb, clean=False):
    return (1 if tf else 0) + 2 * dense + 6 * majb + (18 if clean else 0)


def _accepted(r, what, forms, items):
    """the forms of `forms` the scene serves (a refusal is a VolrenError that says why)"""
    import volren_amd
    ok = []
    for f in forms:
        try:
            r.probe(what, f, items[:1])
            ok.append(f)
        except volren_amd.VolrenError as e:
            assert "cannot serve" in str(e), e
    return ok


def _grid_probes(r, o, lut, paired, voxels=None, majorants=True, tri_n=1 << 14):
    """voxel, trilinear and majorant probes in every form the scene serves; `voxels`: the voxel items of the density grid (default: the whole box + a ring of 2)"""
    dense = o.density.dense is not None
    nb = o.density.n_bricks
    ext = tuple(o.density.extent) if dense else tuple(8 * n for n in nb)
    vox = lc.voxel_box(ext) if voxels is None else voxels
    tri = lc.trilinear_points(ext, n=tri_n)
    for d in ((1, 2) if dense else (0, 2)):
        _check(r, o, lc.VOXEL, d, vox)
        _check(r, o, lc.TRILINEAR, d, tri)
        if lut and not dense and r.tf_float_atlas:
            _check(r, o, lc.TRILINEAR, d + 6, tri)                       # the decoded float atlas (decode_atlas_kernel)
    if o.emission is not None:
        evox = vox.copy()
        evox[:, 0] = 1
        edense = o.emission.dense is not None
        _check(r, o, lc.VOXEL, 2, evox)
        etri = tri.copy()
        etri[:, 0] = 1
        _check(r, o, lc.TRILINEAR, 2, etri)
        assert _accepted(r, lc.VOXEL, (3,), vox) == ([3] if paired else [])
        if paired:
            _check(r, o, lc.VOXEL, 3, vox)                               # pair_atlas_kernel's density half
            _check(r, o, lc.VOXEL, 6, evox)                              # ... and its emission half
            _check(r, o, lc.TRILINEAR, 3, tri)
        elif not edense and not dense:
            _check(r, o, lc.VOXEL, 0, evox)
    if majorants:
        mj = lc.majorant_cells(nb)
        layout = _accepted(r, lc.MAJORANT, [_maj_form(lut, 1 if dense else 0, m) for m in ((0,) if dense else (0, 1))], mj)
        assert len(layout) == 1, layout                                  # the table is in exactly one layout, and the probe knows which
        _check(r, o, lc.MAJORANT, layout[0], mj)
        _check(r, o, lc.MAJORANT, layout[0] + 18, lc.majorant_cells(nb, clean=True))
        _check(r, o, lc.MAJORANT, _maj_form(lut, 2, 2), mj)
        assert _accepted(r, lc.MAJORANT, (_maj_form(not lut, 2, 2),), mj) == []
    if lut:
        _check(r, o, lc.TF, 0, lc.tf_densities())


def _opaque_lut():
    rs = np.random.RandomState(5)
    lut = rs.uniform(0, 1, (16, 4)).astype(np.float32)
    lut[:, 3] = np.sort(lut[:, 3])[::-1]
    return lut


def _set_lut(o, r, lut):
    if lut == "file":
        o.load_transferfunc(scenes.LUT)
        r.load_transferfunc(scenes.LUT)
        o.show_environment = True
    elif lut == "opaque":
        for x in (o, r):
            x.set_transferfunc(_opaque_lut())
            x.tf_window_left, x.tf_window_width = -0.2, 0.9


@pytest.mark.parametrize("lut", [None, "file", "opaque"])
def test_smoke_brick(lut):
    """smoke.brick exhaustively, with and without a LUT (one whose "outside" majorant is not 0), density scales 1, 2^-16, 2^24, float atlas on and off"""
    o, r = scenes.oracle_scene("c2", 32, 32), scenes.hip_scene("c2", 32, 32)
    _set_lut(o, r, lut)
    for scale in (1.0, 2.0 ** -16, 2.0 ** 24):
        o.density_scale = r.density_scale = scale
        _grid_probes(r, o, lut is not None, False)
    if lut:
        r.tf_float_atlas = 0
        assert _accepted(r, lc.TRILINEAR, (6,), lc.trilinear_points((8, 8, 8), n=8)) == []
        _grid_probes(r, o, True, False, majorants=False)


@pytest.mark.parametrize("nbc", [(5, 3, 7), (1, 2, 1), (8, 7, 3)])
def test_ragged_brick_counts(nbc):
    import encoder_ref
    import volren_amd
    from oracle import binding as ob
    a = scenes.crop_bricks(encoder_ref.encode_arrays(scenes.synthetic_density(64)), nbc)
    r = volren_amd.Renderer(32, 32)
    r.load_envmap(scenes.HDR)
    r.set_volume_brick(a["transform"], a["n_bricks"], a["min_maj"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"], commit=True)
    g = ob.Grid()
    g.set(a["transform"], a["n_bricks"], a["min_maj"], a["brick_counter"], a["indirection"], a["rng"], a["atlas_dim"], a["atlas"], a["mips"])
    o = ob.OracleRenderer(32, 32)
    o.load_envmap(scenes.HDR)
    o.set_volume(g)
    _grid_probes(r, o, False, False)
    _set_lut(o, r, "opaque")
    _grid_probes(r, o, True, False)


def test_dense_fp16_ragged_extent():
    """a dense fp16 grid whose extents are no multiples of 4: the voxel array itself is the reference of the DENSE = 1 form"""
    import encoder_ref
    import volren_amd
    from oracle import binding as ob
    dens = scenes.synthetic_density(44)[:37, :30, :43].copy()
    r = volren_amd.Renderer(32, 32)
    r.load_envmap(scenes.HDR)
    r.set_volume_dense_f16(dens)
    o = ob.OracleRenderer(32, 32)
    o.load_envmap(scenes.HDR)
    o.set_volume(encoder_ref.encode_dense_fp16(dens))
    _grid_probes(r, o, False, False)
    got = r.probe(lc.VOXEL, 1, lc.voxel_box((43, 30, 37), ring=0))[:, 0].reshape(37, 30, 43)
    assert lc.same(got, dens.astype(np.float16).astype(np.float32))
    _set_lut(o, r, "file")
    _grid_probes(r, o, True, False)


@pytest.mark.parametrize("name", ["c4:64", "c5:64", "c5cloud:128"])
@pytest.mark.parametrize("lut", [None, "file"])
def test_synthetic_configs_small_exhaustive(name, lut):
    """BASELINE configs[3] / [4] at a small size, exhaustively: the device brick encoder (c5), the paired atlas in both majorant layouts (c5, c5cloud), dense (c4)"""
    o, r = scenes.oracle_scene(name, 32, 32), scenes.hip_scene(name, 32, 32)
    _set_lut(o, r, lut)
    paired = not name.startswith("c4")
    for layout in ((0, 1) if paired else (-1,)):
        r.majorant_layout = layout
        if paired:
            assert r.majorant_blocked == layout                      # the setter took effect: the two rounds probe two layouts
            assert _accepted(r, lc.MAJORANT, [_maj_form(lut is not None, 0, m) for m in (0, 1)], lc.majorant_cells(o.density.n_bricks)[:1]) == [_maj_form(lut is not None, 0, layout)]
        _grid_probes(r, o, lut is not None, paired)
    if paired:                                        # an environment that fails the division check: no kernel reads the paired atlas, the PAIR forms are refused
        for x in (o, r):
            x.set_envmap(lc.dark_patch_map())
        _grid_probes(r, o, lut is not None, False, majorants=False)


def test_emission_grid_with_another_brick_layout():
    """density 40^3 and temperature 40 x 40 x 72: no paired atlas, every grid read from its own"""
    import volren_amd
    import encoder_ref
    from oracle import binding as ob
    dens = scenes.synthetic_density(40)
    temp = np.clip(dens * 0.2 + 0.1 * scenes.synthetic_density(40, seed=99), 0, None).astype(np.float32)
    temp = np.concatenate([temp, temp[:, :, :32]], 2)
    r = volren_amd.Renderer(32, 32)
    r.load_envmap(scenes.HDR)
    r.set_volume_dense(dens, commit=False)
    r.set_volume_dense(temp, name="temperature", commit=True)
    gd, gt = encoder_ref.encode(dens), encoder_ref.encode(temp)
    gd.extent = (40, 40, 40); gd.c.extent[:] = gd.extent
    gt.extent = (72, 40, 40); gt.c.extent[:] = gt.extent
    o = ob.OracleRenderer(32, 32)
    o.load_envmap(scenes.HDR)
    o.set_volume(gd, emission=gt, majorant_emission=float(temp.max()))
    o.density_scale = r.density_scale = 50.0
    assert r.kernel_variant == 3
    nb = o.density.n_bricks
    vox = lc.voxel_box(tuple(8 * n for n in nb))
    _grid_probes(r, o, False, False, voxels=vox)
    evox = lc.voxel_box(tuple(8 * n for n in o.emission.n_bricks), grid=1)
    _check(r, o, lc.VOXEL, 2, evox)
    _check(r, o, lc.VOXEL, 0, evox)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["c4:512", "c5full", "c5cloud"])
def test_full_size_grids(name):
    """512^3 dense / 1024^3 sparse grids: every majorant cell of every level (2.4 M), and the voxels of the structured set -- first and last voxel of the first and
    last brick, the highest brick index on each axis, every brick of the last z layer -- plus 2^20 seeded random voxels; the 32-bit line index of a tap
    (vr_trace.h tap_load) at the highest brick indices included."""
    o, r = scenes.oracle_scene(name, 32, 32), scenes.hip_scene(name, 32, 32)
    nb = o.density.n_bricks
    paired = not name.startswith("c4")
    _grid_probes(r, o, False, paired, voxels=lc.voxel_set(nb), tri_n=1 << 16)
    if paired:
        r.majorant_layout = 1 - r.majorant_blocked
        _grid_probes(r, o, False, True, voxels=lc.voxel_set(nb, n_random=1 << 16), tri_n=1 << 12)


ENV_MAPS = {
    "hdr": lambda: None,
    "rgbe1x1": lambda: lc.rgbe_map(1, 1), "rgbe2x1": lambda: lc.rgbe_map(2, 1), "rgbe3x2": lambda: lc.rgbe_map(3, 2), "rgbe33x17": lambda: lc.rgbe_map(33, 17),
    "float3x2": lambda: lc.nudged(lc.rgbe_map(3, 2)), "float33x17": lambda: lc.nudged(lc.rgbe_map(33, 17)),
    "rgbe511x257": lambda: lc.rgbe_map(511, 257), "rgbe4100x3": lambda: lc.rgbe_map(4100, 3),
    "dark_patch": lc.dark_patch_map, "black": lambda: np.zeros((4, 8, 3), np.float32), "one_lit": lc.one_lit_map,
}


@pytest.mark.parametrize("name", sorted(ENV_MAPS))
def test_environment_lookups(name):
    """impmap_base_kernel / impmap_mip_kernel / env_cdf_kernel and the compact map against the oracle: every importance texel of every level; texel centres, edges,
    special coordinates and 2^20 random points in float and compact form; sky directions; light samples -- one targeted draw per base-level texel, the thresholds of
    the three coarsest levels +- one ulp, a 1024^2 lattice -- by both samplers (the div_core one is refused on the map that fails the division check).
    Coverage of the targeted draws, as the oracle alone resolves them: at least 99 % of the lit texels; the dark-patch map is exempt (1e-30 texels no float32
    draw reaches) and held to the oracle's own share, 253 952 / 262 144 = 0.96875."""
    env = ENV_MAPS[name]()
    o, r = scenes.oracle_scene("c2", 32, 32), scenes.hip_scene("c2", 32, 32)
    if env is not None:
        for x in (o, r):
            x.set_envmap(env)
    o.env_strength = r.env_strength = 1.7
    o.set_env_rot(33.0)
    r.env_rot = 33.0
    compact = name.startswith("rgbe") or name in ("hdr", "black", "one_lit")
    assert r.env_compact == int(compact) and r.env_div_safe == int(name != "dark_patch")
    h, w = o.env_tex.shape[:2]
    _check(r, o, lc.IMPORTANCE, 0, lc.importance_all())
    avg = o.probe(lc.IMPORTANCE, np.array([[0, 0, 9, 0]], np.int32))
    for form in (1, 2):
        assert lc.same(r.probe(lc.IMPORTANCE, form, np.zeros((1, 4), np.int32)), avg)
    tex = lc.texel_points(w, h)
    _check(r, o, lc.TEXEL, 0, tex)
    assert _accepted(r, lc.TEXEL, (1,), tex) == ([1] if compact else [])
    if compact:
        _check(r, o, lc.TEXEL, 1, tex)
    _check(r, o, lc.SKY, 0, lc.sky_directions())
    forms = _accepted(r, lc.LIGHT, (0, 1), lc.light_lattice(2))
    assert forms == ([0, 1] if name != "dark_patch" else [1])
    sets = [lc.light_thresholds(o.impmap), lc.light_lattice(1024)]
    base = lc._levels(o.impmap)[0]
    if (base > 0).any():
        items, tx, ty = lc.light_targeted(o.impmap)
        sets.append(items)
        _, hit = o.probe(lc.LIGHT, items, texel=True)
        lit = int((base > 0).sum())
        share = ((hit[:, 0] == tx) & (hit[:, 1] == ty) & (base[ty, tx] > 0)).sum() / lit
        assert share >= (0.96875 if name == "dark_patch" else 0.99), "targeted draws reach %.4f of the %d lit texels" % (share, lit)
    for items in sets:
        for form in forms:
            _check(r, o, lc.LIGHT, form, items)


# ---- no table is stale ------------------------------------------------------------------------------------------------------------------------------
def _subset(items, n=1 << 16, seed=1):
    if len(items) <= n:
        return items
    return items[np.random.RandomState(seed).choice(len(items), n, replace=False)]


def _all_probes(r, lut, dense, emission, compact, ext, nb):
    """every probe the state can serve, on fixed 2^16-item subsets: a dict of outputs"""
    out = {}
    vox = _subset(lc.voxel_box(ext))
    tri = lc.trilinear_points(ext, n=1 << 13)
    d = 1 if dense else 0
    out["voxel"] = r.probe(lc.VOXEL, 2, vox)
    out["voxel-d"] = r.probe(lc.VOXEL, d, vox)
    out["tri"] = r.probe(lc.TRILINEAR, 2, tri)
    if _accepted(r, lc.TRILINEAR, (6,), tri):
        out["tri-f32"] = r.probe(lc.TRILINEAR, 6, tri)
    if emission:
        evox = vox.copy()
        evox[:, 0] = 1
        out["evoxel"] = r.probe(lc.VOXEL, 2, evox)
        if _accepted(r, lc.VOXEL, (3,), vox):
            out["pair-d"], out["pair-e"] = r.probe(lc.VOXEL, 3, vox), r.probe(lc.VOXEL, 6, evox)
    mj = _subset(lc.majorant_cells(nb))
    out["maj"] = r.probe(lc.MAJORANT, _maj_form(lut, 2, 2), mj)
    for f in _accepted(r, lc.MAJORANT, [_maj_form(lut, d, m) for m in (0, 1)], mj):
        out["maj-own"] = r.probe(lc.MAJORANT, f, mj)
    if lut:
        out["tf"] = r.probe(lc.TF, 0, lc.tf_densities(1 << 12))
    out["imp"] = r.probe(lc.IMPORTANCE, 0, _subset(lc.importance_all()))
    out["avg"] = r.probe(lc.IMPORTANCE, 1, np.zeros((1, 4), np.int32))
    tex = _subset(lc.texel_points(33, 17, n_random=1 << 14))
    out["texel"] = r.probe(lc.TEXEL, 0, tex)
    if compact:
        out["texel-c"] = r.probe(lc.TEXEL, 1, tex)
    out["sky"] = r.probe(lc.SKY, 0, lc.sky_directions(1 << 12))
    for f in _accepted(r, lc.LIGHT, (0, 1), lc.light_lattice(2)):
        out["light%d" % f] = r.probe(lc.LIGHT, f, lc.light_lattice(256))
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("render_between", [False, True])
def test_no_table_is_stale(render_between):
    """A renderer walked through state changes -- with no render in between, then with one render(1) between the steps -- answers every probe like a renderer
    created fresh in that state: density scale, LUT upload / other values / removed, transfer-function window, majorant layout, float atlas off and on, environment
    compact -> float -> compact, animation frame forth and back, encoder toggled with a re-commit, a second volume of another brick count, emission grid added
    and removed.  RendererHIP::MajKey names what the majorant table is keyed on; this is what says the key is complete."""
    import volren_amd
    d0, d1 = scenes.synthetic_density(40), scenes.synthetic_density(40, seed=77)
    t0 = np.clip(d0 * 0.2, 0, None).astype(np.float32)
    big = scenes.synthetic_density(72)[:60, :52, :70].copy()
    lut_a = np.loadtxt(scenes.LUT, delimiter=",", dtype=np.float32)
    lut_b = np.ascontiguousarray(lut_a[::-1] * np.float32(0.5))
    env_c, env_f = lc.rgbe_map(33, 17), lc.nudged(lc.rgbe_map(33, 17))

    state = dict(frames=[d0, d1], temp=None, frame=0, scale=30.0, lut=None, window=(0.0, 1.0), layout=-1, float_atlas=1, env=env_c, encoder=1)

    def build(r, st):
        r.gpu_encoder = st["encoder"]
        r.set_envmap(st["env"])
        r.set_volume_dense(st["frames"][0], commit=False)
        for f in st["frames"][1:]:
            r.volume_add_grid_frame(f)
        if st["temp"] is not None:
            for i in range(len(st["frames"])):
                r.volume_update_grid_frame(i, st["temp"], name="temperature")
        r.commit()
        apply(r, st)

    def apply(r, st):
        r.grid_frame_counter = st["frame"]
        r.density_scale = st["scale"]
        r.set_transferfunc(st["lut"])
        if st["lut"] is not None:                          # (the window belongs to the transfer function: there is none to set it on otherwise)
            r.tf_window_left, r.tf_window_width = st["window"]
        r.majorant_layout = st["layout"]
        r.tf_float_atlas = st["float_atlas"]

    def probes(r, st):
        shape = st["frames"][st["frame"]].shape
        ext = (shape[2], shape[1], shape[0])
        nb = tuple((e + 7) // 8 for e in ext)
        nb = tuple((n + 7) // 8 * 8 for n in nb)
        return _all_probes(r, st["lut"] is not None, False, st["temp"] is not None, st["env"] is env_c, tuple(8 * n for n in nb), nb)

    walked = volren_amd.Renderer(32, 32)
    build(walked, state)
    steps = [
        ("density scale", dict(scale=7.5)),
        ("LUT upload", dict(lut=lut_a)),
        ("LUT of the same size, other values", dict(lut=lut_b)),
        ("transfer-function window", dict(window=(-0.1, 0.7))),
        ("window left alone", dict(window=(-0.3, 0.7))),
        ("window width alone", dict(window=(-0.3, 1.4))),
        ("density scale under a LUT", dict(scale=9.0)),
        ("float atlas off", dict(float_atlas=0)),
        ("float atlas on", dict(float_atlas=1)),
        ("LUT removed", dict(lut=None)),
        ("environment float", dict(env=env_f)),
        ("environment compact", dict(env=env_c)),
        ("frame 1", dict(frame=1)),
        ("frame 0", dict(frame=0)),
        ("emission grid added", dict(temp=t0)),
        ("majorant layout 1", dict(layout=1)),
        ("majorant layout 0", dict(layout=0)),
        ("majorant layout -1", dict(layout=-1)),
        ("LUT with an emission grid", dict(lut=lut_a)),
        ("window under that LUT", dict(window=(0.05, 0.6))),
        ("density scale under that LUT", dict(scale=12.0)),
        ("host encoder, re-commit", dict(encoder=0)),
        ("device encoder, re-commit", dict(encoder=1)),
        ("emission grid removed", dict(temp=None)),
        ("a volume of another brick count", dict(frames=[big], frame=0)),
        ("density scale on the new volume", dict(scale=55.0)),
    ]
    def walk(r, st, change):
        """only what the step changes is applied to the walked renderer: a LUT that is not in the step is NOT uploaded again (an upload gets a new
        TransferFunction::version, which alone would rebuild the majorant table whatever else its key holds)"""
        if "env" in change:
            r.set_envmap(st["env"])
        if any(k in change for k in ("frames", "temp", "encoder")):
            r.gpu_encoder = st["encoder"]
            if "frames" in change or change.get("temp", 0) is None:
                # a second set_volume: the volume is replaced (and with it the temperature grids); it moves the volume to the unit cube, which sets the
                # density scale, so the scale is set again -- to the value it had: no key field changes but what set_volume / commit themselves reset
                r.set_volume_dense(st["frames"][0], commit=False)
                for f in st["frames"][1:]:
                    r.volume_add_grid_frame(f)
            if st["temp"] is not None:
                for i in range(len(st["frames"])):
                    r.volume_update_grid_frame(i, st["temp"], name="temperature")
            r.commit()
            if "frames" in change or change.get("temp", 0) is None:
                r.density_scale = st["scale"]
                r.grid_frame_counter = st["frame"]
        if "frame" in change and "frames" not in change:
            r.grid_frame_counter = st["frame"]
        if "scale" in change:
            r.density_scale = st["scale"]
        if "lut" in change:
            r.set_transferfunc(st["lut"])
        if st["lut"] is not None and ("lut" in change or "window" in change):      # (a new transfer function starts with its own window)
            r.tf_window_left, r.tf_window_width = st["window"]
        if "layout" in change:
            r.majorant_layout = st["layout"]
        if "float_atlas" in change:
            r.tf_float_atlas = st["float_atlas"]

    for what, change in steps:
        if render_between:
            walked.render(1)
        state.update(change)
        walk(walked, state, change)
        fresh = volren_amd.Renderer(32, 32)
        build(fresh, state)
        got, want = probes(walked, state), probes(fresh, state)
        assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
        for k in want:
            assert lc.same(got[k], want[k]), "after '%s': probe %s differs from a fresh renderer in %d items" % (
                what, k, int((~((lc.bits(got[k]) == lc.bits(want[k])) | (np.isnan(got[k]) & np.isnan(want[k]))).all(-1)).sum()))
        fresh.close()


# ---- the device brick encoder on hostile inputs -----------------------------------------------------------------------------------------------------
def _encoded_pair(dens):
    """dens through the device encoder and through the host encoder: two renderers, density scale 1"""
    import volren_amd
    out = []
    for gpu in (1, 0):
        r = volren_amd.Renderer(32, 32)
        r.gpu_encoder = gpu
        r.load_envmap(scenes.HDR)
        r.set_volume_dense(dens)
        r.density_scale = 1.0
        out.append(r)
    return out


def _reference_of(dens):
    import encoder_ref
    from oracle import binding as ob
    g = encoder_ref.encode(dens)
    g.extent = tuple(dens.shape[::-1])
    g.c.extent[:] = g.extent
    o = ob.OracleRenderer(32, 32)
    o.load_envmap(scenes.HDR)
    o.set_volume(g)
    o.density_scale = 1.0
    return o


@pytest.mark.parametrize("kind,extent", scenes.HOSTILE_CASES, ids=["%s-%dx%dx%d" % ((k,) + e) for k, e in scenes.HOSTILE_CASES])
def test_device_encoder_on_hostile_inputs(kind, extent):
    """encode_range_kernel / encode_brick_kernel / range_mip_kernel against the host encoder (checksums of records, atlas and range mips) AND both against the
    numpy reference encoder through the probes -- every voxel of the padded extent plus a ring of 2, every majorant cell of every level -- on constant, negative,
    beyond-fp16, tiny, denormal, spiky, tie and +inf data and on extents of one voxel, one brick layer, and with bricks fully outside the data."""
    dens = scenes.hostile_dense(kind, extent)
    dev, host = _encoded_pair(dens)
    assert dev.grid_checksums() == host.grid_checksums(), (kind, extent)
    o = _reference_of(dens)
    for r in (dev, host):
        _grid_probes(r, o, False, False, tri_n=1 << 10)


def test_device_encoder_minus_zero_voxels():
    """-0.0 voxels.  -0.0 and +0.0 compare equal, so which of them a minimum search ends on depends on its order: the host encoder's loop and the device
    encoder's wavefront reduction gave range words that differed in the sign bit (a majorant of -0.0 on one side) until both -- and encoder_ref -- made a zero range
    bound +0.0.  Pinned between the two encoders bit for bit, and by value: decoded voxels and majorants numerically equal to the reference's."""
    for extent in ((65, 9, 8), (3, 70, 1)):
        dens = scenes.hostile_dense("minus_zero", extent)
        dev, host = _encoded_pair(dens)
        assert dev.grid_checksums() == host.grid_checksums(), extent
        o = _reference_of(dens)
        nb = o.density.n_bricks
        vox, mj = lc.voxel_box(tuple(8 * n for n in nb)), lc.majorant_cells(nb)
        for what, items in ((lc.VOXEL, vox), (lc.MAJORANT, mj)):
            want = o.probe(what, items)
            got_d, got_h = dev.probe(what, 2 if what == lc.VOXEL else _maj_form(False, 2, 2), items), host.probe(what, 2 if what == lc.VOXEL else _maj_form(False, 2, 2), items)
            assert lc.same(got_d, got_h)
            assert np.array_equal(got_d, want)                          # numerically: -0.0 == 0.0


def test_device_encoder_nan_voxels():
    """NaN voxels.  Both encoders leave a NaN out of a brick's range (`v < lo ? v : lo`) and quantise it to a DEFINED 0 (the clamp is written so that a NaN takes
    its lower branch; a conversion of NaN to uint8_t would be undefined in C++): a NaN voxel decodes to its brick's range minimum.  Pinned between
    the two encoders bit for bit, and against encoder_ref, which states the same rule (nanmin / nanmax, NaN -> 0); a 12^3 window of NaN only is not defined."""
    for extent in ((65, 9, 8), (129, 8, 8)):
        dens = scenes.hostile_dense("nan", extent)
        assert np.isnan(dens).any()
        dev, host = _encoded_pair(dens)
        assert dev.grid_checksums() == host.grid_checksums(), extent
        o = _reference_of(dens)
        for r in (dev, host):
            _grid_probes(r, o, False, False, tri_n=1 << 10)
        nz, ny, nx = dens.shape
        got = dev.probe(lc.VOXEL, 0, lc.voxel_box((nx, ny, nz), ring=0))[:, 0].reshape(nz, ny, nx)
        assert not np.isnan(got).any()                                  # what a caller gets: a finite value, the minimum of the brick's range
