"""One committed walk of a LIVE renderer through scene, camera and switch changes, and what every read-back must return after each step -- computed without the
product: the oracle's frame, the host builds of the tile classifiers (hk_sky, hk_see_through) and of the guide passes (hk_features, hk_expected_cubic), the numpy
statement of the clear-distance tables.  tests/test_walk_host.py holds the catalogue itself (no step is vacuous, every step back is a real return, the walk reaches
what it claims); tests/test_gpu_walk.py walks a renderer through it.  TEST HARNESS ONLY.

What the walk is after: RendererHIP keeps derived state alive across changes, each under a hand-written rule for when it is stale -- the march / clear /
see-through tile lists (split_tiles, split_key_), the costliest-first order (tile_order, order_key_), a grid's live cells (split_three), its clear-distance tables of
reach 1 and 2 (clear_table_of), the majorant tables (MajKey), the decoded float atlas and the paired atlas (capture), the path-seed table (seed_table_*), the
recorded trace() calls (LaunchInputs::same_launch_as).

A state is a plain dict (START).  Arrays are named: a state holds the NAME of a LUT, an environment map or a dense frame (data()), so that states compare and hash.
A step is (name, change, targets, straddle): `change` holds the fields that get new values, `targets` the read-backs the step is meant to move, `straddle` says
that the change does not restart the frame (tests/test_gpu_walk.py records trace() calls on both sides of it)."""
import functools

import numpy as np

import hk_expected_cubic as hc
import hk_features
import hk_see_through as st
import hk_sky
import lookup_cases as lc
import scenes
from oracle import binding as ob

READ_BACKS = ("frame", "classes", "features", "expected0", "expected1", "table1", "table2")
SPP, FEATURE_SPP, RAYS = 4, 3, 2
ANIMATION_SCALE = 40.0          # density scale of the 40^3 blob frames (voxels in [0, 1]); tests/test_gpu_expected_skip.py renders them with the same


def _blob(n, cx, cy, cz, rad):
    """the frames of tests/test_gpu_expected_skip.py::test_a_table_never_outlives_its_grid"""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.maximum(0.0, 1.0 - ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (rad * rad)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def data(name):
    """the array behind a name a state holds; read-only"""
    if name == "blob_a":
        a = _blob(40, 9.0, 9.0, 9.0, 7.0)
    elif name == "blob_b":
        a = _blob(40, 30.0, 30.0, 30.0, 7.0)
    elif name == "blob_c":
        a = _blob(40, 30.0, 9.0, 20.0, 7.0)
    elif name == "blob_c64":                                # blob_c in the 64^3 voxels a .brick frame of the 40^3 blobs spans (8^3 bricks): the same box
        a = np.zeros((64, 64, 64), np.float32)
        a[:40, :40, :40] = _blob(40, 30.0, 9.0, 20.0, 7.0)
    elif name == "temp_a":                                  # an emission grid over blob_a's smoke, same brick layout
        a = (_blob(40, 9.0, 9.0, 9.0, 5.0) * np.float32(0.5)).astype(np.float32)
    elif name == "lut_file":
        a = np.loadtxt(scenes.LUT, delimiter=",", dtype=np.float32)
    elif name == "env_float":                               # not representable in the compact form (tests/test_gpu_lookups.py::test_no_table_is_stale)
        a = lc.nudged(lc.rgbe_map(33, 17))
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _start():
    o = scenes.oracle_scene("c2", 72, 56)                   # BASELINE configs[1]: smoke.brick, the .hdr sky, 100 bounces, fov 40
    return dict(
        size=(72, 56), cam_pos=tuple(o.cam_pos), cam_dir=tuple(o.cam_dir), cam_fov=40.0, vol_clip_min=(0.0, 0.0, 0.0), vol_clip_max=(1.0, 1.0, 1.0),
        density_scale=float(o.density_scale), seed=42,
        volume="smoke", grid_frame_counter=0, temperature=None,          # volume: "smoke" (the file) or a tuple of frames: "NAME" a dense float grid,
                                                                         # "brick:NAME" the same voxels as a .brick file of a folder of frames
        lut=None, window=(0.0, 1.0), integrator=0, show_environment=1, env_strength=1.0, env_rot=0.0, env="hdr",
        tiles=None,                                                      # None: the whole frame; else a tuple of tile ids
        sky_tiles=1, see_through_tiles=1, order_tiles=1, seed_table_mb=-1, seed_table_max_samples=0, fast_math=0,
        stream=None)                                                     # None: the default stream; else the name of a caller's stream


START = _start()
SMOKE_SCALE = START["density_scale"]


def _unit(v):
    v = np.array(v, np.float32)
    return tuple(float(x) for x in v / np.float32(np.sqrt(np.float32(v @ v))))


TURNED = (-0.9, 0.35, 1.05)
AWAY = _unit((-0.158, -0.245, -0.956))          # from TURNED: 50 degrees off the volume about the y axis
SUBSET_A = (0, 1, 2, 5, 6, 7, 10, 11)              # the frame's lower left: a clear corner, march tiles -- no see-through tile
SUBSET_B = (19, 18, 17, 14, 13, 12, 9, 4)          # the upper right, in falling order: two clear corners and the see-through tile


def S(name, change, targets=(), straddle=False):
    assert set(targets) <= set(READ_BACKS), targets
    return (name, change, frozenset(targets), straddle)


_IMAGE = ("frame", "features", "expected0", "expected1")
_VIEW = _IMAGE + ("classes",)
_FRAMES = _IMAGE + ("table1", "table2")
_GRID = _VIEW + ("table1", "table2")

STEPS = [
    # ---- camera and box ----
    S("camera turned about the volume", dict(cam_pos=TURNED, cam_dir=_unit([-c for c in TURNED])), _VIEW, True),
    S("fov 25", dict(cam_fov=25.0), _VIEW, True),
    S("see_through_tiles 0", dict(see_through_tiles=0), ("classes",), True),
    S("seed 7", dict(seed=7), ("frame", "features"), True),
    S("camera looks away", dict(cam_dir=AWAY), _VIEW, True),                     # the box in front of the camera and outside the frame: every tile is clear
    S("fov 70", dict(cam_fov=70.0), _VIEW, True),
    S("camera inside the box", dict(cam_pos=(0.02, 0.01, 0.03), cam_dir=_unit((0.3, 0.2, -1.0))), _VIEW, True),
    S("fov 40", dict(cam_fov=40.0), _IMAGE, True),
    S("camera back", dict(cam_pos=START["cam_pos"], cam_dir=START["cam_dir"]), _VIEW, True),
    S("see_through_tiles 1", dict(see_through_tiles=1), ("classes",), True),
    S("seed 42", dict(seed=42), ("frame", "features"), True),
    S("camera moved back along its direction", dict(cam_pos=(1.5, 0.0, 1.5)), _VIEW, True),          # cam_pos alone: the direction stays
    S("camera moved forward again", dict(cam_pos=START["cam_pos"]), _VIEW, True),
    S("clip box x in [0.25, 0.75]", dict(vol_clip_min=(0.25, 0.0, 0.0), vol_clip_max=(0.75, 1.0, 1.0)), _VIEW, True),
    S("order_tiles 2", dict(order_tiles=2), (), True),
    S("clip box whole", dict(vol_clip_min=(0.0, 0.0, 0.0), vol_clip_max=(1.0, 1.0, 1.0)), _VIEW, True),
    # ---- frame size and tile subsets ----
    S("resize 128x128", dict(size=(128, 128)), _VIEW),
    S("order_tiles 0", dict(order_tiles=0), (), True),
    S("resize 72x56", dict(size=(72, 56)), _VIEW),
    S("tile subset A", dict(tiles=SUBSET_A), _VIEW),
    S("order_tiles 1", dict(order_tiles=1), (), True),
    S("tile subset B of the same length", dict(tiles=SUBSET_B), _VIEW),
    S("sky_tiles 0", dict(sky_tiles=0), ("classes",), True),
    S("the whole frame", dict(tiles=None), _IMAGE),
    S("sky_tiles 1", dict(sky_tiles=1), ("classes",), True),
    # ---- density scale ----
    S("density scale halved", dict(density_scale=SMOKE_SCALE * 0.5), _IMAGE),
    S("seed_table_mb 0", dict(seed_table_mb=0), (), True),
    S("density scale 2^-17", dict(density_scale=2.0 ** -17), _IMAGE),
    S("seed_table_mb -1", dict(seed_table_mb=-1), (), True),
    S("density scale back", dict(density_scale=SMOKE_SCALE), _IMAGE),
    # ---- transfer function and integrators ----
    S("integrator 1", dict(integrator=1), ("frame",), True),
    S("integrator 0", dict(integrator=0), ("frame",), True),
    S("LUT uploaded", dict(lut="lut_file", window=(0.0, 1.0)), _VIEW + ("table2",)),         # (under a LUT field 1 marches the trilinear field: reach 1)
    S("window changed", dict(window=(-0.1, 0.7)), _IMAGE),
    S("integrator 2 under the LUT", dict(integrator=2), ("frame", "classes")),
    S("integrator 0 under the LUT", dict(integrator=0), ("frame", "classes")),
    S("LUT removed", dict(lut=None, window=(0.0, 1.0)), _VIEW + ("table2",)),
    S("integrator 3", dict(integrator=3), ("frame", "classes")),
    S("integrator 0 again", dict(integrator=0), ("frame", "classes")),
    # ---- environment ----
    S("show_environment 0", dict(show_environment=0), ("frame",), True),
    S("env_rot 33", dict(env_rot=33.0), ("frame",), True),
    S("show_environment 1", dict(show_environment=1), ("frame",), True),
    S("env_strength 1.7", dict(env_strength=1.7), ("frame",)),
    S("seed_table_max_samples 2", dict(seed_table_max_samples=2), ()),
    S("environment float", dict(env="env_float"), ("frame",)),
    S("env_rot 0", dict(env_rot=0.0), ("frame",), True),
    S("environment compact", dict(env="hdr"), ("frame",)),
    S("seed_table_max_samples 0", dict(seed_table_max_samples=0), ()),
    S("env_strength 1", dict(env_strength=1.0), ("frame",)),
    # ---- tolerance mode and streams ----
    S("fast_math 1", dict(fast_math=1), ("classes",)),
    S("fast_math 0", dict(fast_math=0), ("classes",)),
    S("a caller's stream", dict(stream="s1"), ()),
    S("the default stream", dict(stream=None), ()),
    # ---- the volume ----
    S("a two-frame dense animation", dict(volume=("blob_a", "blob_b"), grid_frame_counter=0, density_scale=ANIMATION_SCALE), _GRID),
    S("grid_frame_counter 1", dict(grid_frame_counter=1), _FRAMES, True),
    S("frame 1 replaced and committed", dict(volume=("blob_a", "blob_c")), _FRAMES),
    S("grid_frame_counter 0", dict(grid_frame_counter=0), _FRAMES, True),
    S("temperature grid added", dict(temperature="temp_a"), ("frame",)),
    S("temperature grid removed", dict(temperature=None), ("frame",)),
    # the same frames as a folder of .brick files: the host holds their range tables, so each frame has see-through tiles of its own
    S("a two-frame brick animation", dict(volume=("brick:blob_a", "brick:blob_b")), _VIEW),
    S("brick frame 1", dict(grid_frame_counter=1), _GRID, True),
    S("brick frame 0", dict(grid_frame_counter=0), _GRID, True),
    S("brick frame 0 replaced by a dense grid and committed", dict(volume=("blob_c64", "brick:blob_b")), _GRID),
    S("smoke.brick again", dict(volume="smoke", grid_frame_counter=0, density_scale=SMOKE_SCALE), _GRID),
]


def states():
    """[(name, change, targets, straddle, state before, state after)] of the whole walk"""
    out, cur = [], dict(START)
    for name, change, targets, straddle in STEPS:
        nxt = dict(cur)
        nxt.update(change)
        out.append((name, change, targets, straddle, cur, nxt))
        cur = nxt
    return out


def key(state):
    return tuple(sorted(state.items(), key=lambda kv: kv[0]))


@functools.lru_cache(maxsize=None)
def brick_folder(names):
    """a folder of .brick frames of the dense grids `names`, in that order, written by the product's host encoder (vr_write_brick_from_dense: no device needed;
    tests/test_lookups_host.py holds it to the numpy reference encoder); removed when the process ends"""
    import atexit
    import os
    import shutil
    import tempfile
    import volren_amd
    folder = tempfile.mkdtemp(prefix="walk_bricks_")
    atexit.register(shutil.rmtree, folder, True)
    lib = volren_amd.load()
    for i, n in enumerate(names):
        a = data(n)
        assert lib.vr_write_brick_from_dense(a.ctypes.data, a.shape[2], a.shape[1], a.shape[0], None, os.path.join(folder, "f%03d.brick" % i).encode()) == 0, lib.vr_last_error()
    return folder


# ---- the product side --------------------------------------------------------------------------------------------------------------------------------
def _set_volume(r, state):
    """the volume from nothing: set_volume moves it to the unit cube, which sets the density scale -- so the scale and the frame counter are set again, to the
    state's values (tests/test_gpu_lookups.py::test_no_table_is_stale does the same)"""
    vol = state["volume"]
    if vol == "smoke":
        r.load_volume(scenes.SMOKE)
    elif any(n.startswith("brick:") for n in vol):                     # a folder of .brick frames, then the frames that are dense grids by now
        assert state["temperature"] is None
        r.load_volume(brick_folder(tuple(n.split(":")[-1] for n in vol)))
        dense = [i for i, n in enumerate(vol) if not n.startswith("brick:")]
        for i in dense:
            r.volume_update_grid_frame(i, data(vol[i]))
        if dense:
            r.commit()
    else:
        frames = [data(n) for n in vol]
        r.set_volume_dense(frames[0], commit=False)
        for f in frames[1:]:
            r.volume_add_grid_frame(f)
        if state["temperature"] is not None:
            for i in range(len(frames)):
                r.volume_update_grid_frame(i, data(state["temperature"]), name="temperature")
        r.commit()
    r.density_scale = state["density_scale"]
    r.grid_frame_counter = state["grid_frame_counter"]


def _set_env(r, state):
    """a new map starts with strength 1 and no rotation: both are set again"""
    if state["env"] == "hdr":
        r.load_envmap(scenes.HDR)
    else:
        r.set_envmap(data(state["env"]))
    r.env_strength = state["env_strength"]
    r.env_rot = state["env_rot"]


_PLAIN = ("cam_pos", "cam_dir", "cam_fov", "vol_clip_min", "vol_clip_max", "seed", "integrator", "show_environment", "env_strength", "env_rot",
          "sky_tiles", "see_through_tiles", "order_tiles", "seed_table_mb", "seed_table_max_samples", "fast_math")


def build_renderer(state, streams=None):
    """a fresh renderer built directly in `state`: the diagnostic that separates "stale" from "wrong" -- never the expectation"""
    import volren_amd
    r = volren_amd.Renderer(*state["size"])
    r.bounces = 100
    r.expected_skip = 1
    _set_volume(r, state)
    apply_change(r, state, {k: state[k] for k in state if k not in ("size", "volume", "grid_frame_counter", "temperature", "density_scale")}, streams)
    return r


def apply_change(r, state, change, streams=None, before=None):
    """Only what the step changes is applied to the renderer `r`; `state` is the state AFTER the step.  A LUT or an environment that is not in the step is NOT
    uploaded again: an upload would itself refresh the caches under test.  streams: {name: stream handle} for the "stream" field.  before: the state the step
    leaves -- with it, frames replaced in a live animation go through update_grid_frame, as a caller would do it."""
    if "size" in change:
        r.resize(*state["size"])
    if "env" in change:
        _set_env(r, state)
    if "volume" in change or "temperature" in change:
        old_frames = None if before is None else before["volume"]
        vol = state["volume"]
        if "volume" in change and vol != "smoke" and old_frames is not None and old_frames != "smoke" and len(old_frames) == len(vol) and "temperature" not in change \
                and state["temperature"] is None and all(a == b or not b.startswith("brick:") for a, b in zip(old_frames, vol)):
            for i, (a, b) in enumerate(zip(old_frames, vol)):           # frames replaced in a live animation: update_grid_frame and commit, nothing else
                if a != b:
                    r.volume_update_grid_frame(i, data(b))
            r.commit()
        elif "volume" not in change and state["temperature"] is not None:      # an emission grid added to every frame of the volume that is there
            for i in range(len(vol)):
                r.volume_update_grid_frame(i, data(state["temperature"]), name="temperature")
            r.commit()
        else:                                                           # another volume, or the emission grids gone: the volume is set anew
            _set_volume(r, state)
    if "grid_frame_counter" in change and "volume" not in change:
        r.grid_frame_counter = state["grid_frame_counter"]
    if "density_scale" in change and "volume" not in change:
        r.density_scale = state["density_scale"]
    if "lut" in change:
        r.set_transferfunc(None if state["lut"] is None else data(state["lut"]))
    if state["lut"] is not None and ("lut" in change or "window" in change):       # (the window belongs to the transfer function; a new one starts with its own)
        r.tf_window_left, r.tf_window_width = state["window"]
    for k in _PLAIN:
        if k in change and not ("env" in change and k in ("env_strength", "env_rot")):
            setattr(r, k, state[k])
    if "tiles" in change:
        r.set_tiles(np.zeros(0, np.int32) if state["tiles"] is None else np.array(state["tiles"], np.int32))
    if "stream" in change:
        r.synchronize()                                                 # the caller's part: nothing of the old stream is in flight when the new one takes over
        r.set_stream(None if state["stream"] is None else streams[state["stream"]])


# ---- the reference side ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid(name):
    """the oracle grid of a frame.  "brick:NAME": the file, read by the oracle's own loader.  A dense float frame: the numpy reference encoder, with the voxel
    extent an in-memory dense grid keeps (scenes.configure_sparse)"""
    import encoder_ref
    if name.startswith("brick:"):
        import os
        return ob.Grid.from_file(os.path.join(brick_folder((name[6:],)), "f000.brick"))
    d = data(name)
    g = encoder_ref.encode(d)
    g.extent = tuple(d.shape[::-1])
    g.c.extent[:] = g.extent
    return g


@functools.lru_cache(maxsize=None)
def _smoke_grid():
    return ob.Grid.from_file(scenes.SMOKE)


def build_oracle(state):
    """an OracleRenderer in `state` (the switches of the product -- tile classes, tile order, seed table, tolerance mode, stream -- are nothing to it)"""
    o = ob.OracleRenderer(*state["size"])
    if state["volume"] == "smoke":
        o.set_volume(_smoke_grid())
    else:
        t = state["temperature"]
        vol, cur = state["volume"], state["volume"][state["grid_frame_counter"]]
        fit = None
        if any(n.startswith("brick:") for n in vol) and not cur.startswith("brick:"):
            # a dense grid that replaced a frame of a loaded folder: the volume keeps the transform load_volume fitted to the folder's frames (64^3 voxels: the
            # host encoder pads 40^3 to 8^3 bricks); update_grid_frame and commit() do not fit it again
            o.set_volume(_grid("brick:" + cur))
            fit = o.volume_transform
        o.set_volume(_grid(cur), emission=None if t is None else _grid(t), majorant_emission=0.0 if t is None else float(data(t).max()))
        if fit is not None:
            o.volume_transform = fit
    o.density_scale = state["density_scale"]
    if state["env"] == "hdr":
        o.load_envmap(scenes.HDR)
    else:
        o.set_envmap(data(state["env"]))
    o.env_strength = state["env_strength"]
    o.set_env_rot(state["env_rot"])
    if state["lut"] is not None:
        o.set_transferfunc(data(state["lut"]))
        o.tf_window_left, o.tf_window_width = state["window"]
    o.bounces = 100
    o.cam_pos, o.cam_dir, o.cam_fov = state["cam_pos"], state["cam_dir"], state["cam_fov"]
    o.vol_clip_min, o.vol_clip_max = state["vol_clip_min"], state["vol_clip_max"]
    o.seed, o.integrator, o.show_environment = state["seed"], state["integrator"], bool(state["show_environment"])
    return o


def tile_ids(state):
    nx, ny = st.tiles_of(*state["size"])
    return np.arange(nx * ny, dtype=np.int32) if state["tiles"] is None else np.array(state["tiles"], np.int32)


def mask(state):
    """[H][W] bool: the pixels of the state's tile set -- what a render() or a guide pass writes; the rest of a buffer keeps what earlier steps left there"""
    w, h = state["size"]
    m = np.zeros((h, w), bool)
    nx = (w + 15) // 16
    for t in tile_ids(state):
        m[(t // nx) * 16:(t // nx) * 16 + 16, (t % nx) * 16:(t % nx) * 16 + 16] = True
    return m


def split_is_on(state):
    """renderer.h LaunchInputs::splits_sky: the clear tiles are split off unless the switch is off, in the tolerance mode, and for the item kernels (integrator 3,
    and 2 under a LUT)"""
    return bool(state["sky_tiles"]) and not state["fast_math"] and not (state["integrator"] == 3 or (state["integrator"] == 2 and state["lut"] is not None))


def host_holds_range_table(state):
    """renderer.cpp commit(): a brick file's table is held; a float grid is encoded on the device, and the host holds no table of it"""
    return state["volume"] == "smoke" or state["volume"][state["grid_frame_counter"]].startswith("brick:")


def tile_classes(state, o=None):
    """(clear tiles, see-through tiles) as last_sky_tiles / last_see_through_tiles must read after a render of the state; the see-through class is empty behind a
    LUT, with an emission grid and for integrators other than 0 and 1 (hk_see_through.classify runs the header's own fallbacks on the oracle's uniforms)"""
    if not split_is_on(state):
        return (0, 0)
    o = o or build_oracle(state)
    ids = tile_ids(state)
    clear = int(hk_sky.classify(o, ids).sum())
    see = 0
    if state["see_through_tiles"]:
        cls, _ = st.classify(o, ids, held=host_holds_range_table(state))
        assert int((cls == st.CLEAR).sum()) == clear
        see = int((cls == st.SEE).sum())
    return (clear, see)


def table_reach(state, field):
    """the table `expected_field` = field marches with: reach 2 for the tracker's cubic field, reach 1 for the trilinear one -- which is also what field 1 marches
    under a LUT (renderer.cpp launch_expected)"""
    return 2 if field == 1 and state["lut"] is None else 1


@functools.lru_cache(maxsize=None)
def _spec_table(grid_name, reach):
    g = _smoke_grid() if grid_name == "smoke" else _grid(grid_name)
    t = hc.spec_table(g, reach)
    t.setflags(write=False)
    return t


_SCENE_FIELDS = ("size", "cam_pos", "cam_dir", "cam_fov", "vol_clip_min", "vol_clip_max", "density_scale", "seed", "volume", "grid_frame_counter", "temperature", "lut",
                 "window", "integrator", "show_environment", "env_strength", "env_rot", "env", "tiles")
_MEMO, _CLASSES = {}, {}


def _scene_references(state, fresh=False):
    """the read-backs the oracle scene alone decides, memoised under the scene's fields (the product's switches are not among them); fresh: computed again"""
    k = tuple((f, state[f]) for f in _SCENE_FIELDS)
    if fresh:
        _MEMO.pop(k, None)
    if k not in _MEMO:
        o = build_oracle(state)
        m = mask(state)
        out = {"frame": o.render(SPP).copy(), "features": hk_features.feature_pass(o, FEATURE_SPP),
               "expected0": hc.expected_pass(o, RAYS, 0)[0], "expected1": hc.expected_pass(o, RAYS, 1)[0]}
        for a in out.values():
            a[~m] = 0                                                  # outside the tile set nothing is held to anything
            a.setflags(write=False)
        name = "smoke" if state["volume"] == "smoke" else state["volume"][state["grid_frame_counter"]]
        out["table1"] = _spec_table(name, table_reach(state, 0))
        out["table2"] = _spec_table(name, table_reach(state, 1))
        _MEMO[k] = out
    return _MEMO[k]


def references(state, fresh=False):
    """{read-back: what it must return in `state`}, computed without the product.  frame, features, expected0 / 1: [H][W][4 | 8] float32, zero outside the state's
    tile set (compare under mask(state)); classes: (clear, see-through); table1 / table2: the clear-distance table under expected_field 0 / 1, uint8 [cz][cy][cx]."""
    out = dict(_scene_references(state, fresh))
    k = key(state)
    if fresh or k not in _CLASSES:
        _CLASSES[k] = tile_classes(state)
    out["classes"] = _CLASSES[k]
    return out


_STRADDLE = {}


def straddle_frame(before, after, n=2):
    """the oracle driven like a trace() loop across a change that does not restart the frame: n samples in `before`, then n more in `after` on the same
    framebuffer; memoised"""
    k = (key(before), key(after), n)
    if k not in _STRADDLE:
        _STRADDLE[k] = _straddle_frame(before, after, n)
        _STRADDLE[k].setflags(write=False)
    return _STRADDLE[k]


def _straddle_frame(before, after, n):
    a = build_oracle(before)
    a.render(n)
    b = build_oracle(after)
    assert b.fb.shape == a.fb.shape
    b.fb[:] = a.fb
    b.sample = a.sample
    b.render(n)
    return b.fb
