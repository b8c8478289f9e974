"""CPU: the clear-tile classifier (volren_amd/csrc/vr_sky_tiles.h) and the primary-miss sample (vr_trace.h sky_sample), built for the host (tests/hk_sky.py).

Soundness: a tile called clear has no hit on a quarter-pixel lattice of slab tests in double over its closed pixel rectangle, and on the small frames the oracle
itself counts nothing but primary misses there.  Tightness: a tile that the same lattice finds clear with a TWO-pixel margin is called clear (the classifier
grows the rectangle by one).  The counts are pinned, so neither condition is vacuous.  sky_sample equals the oracle's trace_pixel_sample bit for bit."""
import numpy as np
import pytest

import hk_sky
import scenes
from hk_common import same
from oracle import binding as ob


def c2(w, h):
    return scenes.oracle_scene("c2", w, h)


def r5(name):
    return lambda: scenes.configure_r5(ob.OracleRenderer(80, 48), name, True)


def cropped():
    r = c2(80, 48)
    r.vol_clip_min, r.vol_clip_max = (0.25, 0.3, 0.25), (0.75, 0.6, 0.8)
    return r


def _box(r):
    p = r.params()
    return np.array(p.vol_bb_min[:], np.float64), np.array(p.vol_bb_max[:], np.float64)


def camera_inside():
    r = c2(80, 48)
    lo, hi = _box(r)
    r.cam_pos = tuple(float(v) for v in 0.5 * (lo + hi) + 0.1 * (hi - lo))
    return r


def box_behind():
    r = c2(80, 48)
    r.cam_dir = tuple(-np.asarray(r.cam_dir, np.float32))          # the default camera looks at the box: now it looks away from it
    return r


def box_straddles():
    r = c2(80, 48)
    r.cam_dir, r.cam_up = (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)         # the box lies beside the camera: its corners on both sides of the camera plane
    lo, hi = _box(r)
    r.cam_pos = (float(hi[0]) + 0.5, 0.5 * float(lo[1] + hi[1]), 0.5 * float(lo[2] + hi[2]))
    return r


# name -> (scene, clear tiles expected or None where the lattice alone decides, degenerate placement)
VIEWS = {
    "c2_1024": (lambda: c2(1024, 1024), 1152),
    "c2_256": (lambda: c2(256, 256), 64),
    "c2_128": (lambda: c2(128, 128), 16),
    "c2_80x48": (lambda: c2(80, 48), 6),
    "c2_72x56": (lambda: c2(72, 56), 4),
    "c2_96x32": (lambda: c2(96, 32), 8),
    "c2_64": (lambda: c2(64, 64), 0),
    "c2_64x48": (lambda: c2(64, 48), 0),
    "r5_cam_b": (r5("cam_b"), None),
    "r5_env_rot": (r5("env_rot"), 6),
    "r5_crop": (r5("crop"), None),
    "cropped": (cropped, None),
    "camera_inside": (camera_inside, 0),
    "box_behind": (box_behind, 0),
    "box_straddles": (box_straddles, 0),
    "c4_64": (lambda: scenes.oracle_scene("c4:64", 256, 256), 0),
}
SMALL = ("c2_80x48", "c2_72x56", "c2_96x32", "r5_cam_b", "r5_crop", "cropped")


@pytest.mark.parametrize("name", list(VIEWS))
def test_clear_tiles_are_sound_and_tight_against_the_lattice(name):
    make, want = VIEWS[name]
    r = make()
    clear = hk_sky.classify(r)
    hits = hk_sky.lattice_hits(r)
    none_hit = hk_sky.lattice_clear(hits, r.w, r.h, 0)
    wide_clear = hk_sky.lattice_clear(hits, r.w, r.h, 2)
    print(name, "clear", int(clear.sum()), "of", clear.size, "| lattice: margin 0", int(none_hit.sum()), "margin 2", int(wide_clear.sum()))
    assert not (clear & ~none_hit).any(), "a tile called clear has a lattice ray that hits the box: %s" % np.flatnonzero(clear & ~none_hit)
    if name not in ("camera_inside", "box_behind", "box_straddles"):           # (the fallback gives up tiles on purpose there)
        assert not (wide_clear & ~clear).any(), "a tile two pixels clear of the box is not called clear: %s" % np.flatnonzero(wide_clear & ~clear)
    if want is not None:
        assert int(clear.sum()) == want
    march, sky = hk_sky.split(r)
    assert np.array_equal(sky, np.flatnonzero(clear)) and np.array_equal(march, np.flatnonzero(~clear))


def test_the_degenerate_placements_really_are_degenerate():
    """the three views the fallback is for: the camera in the box; every corner behind the camera plane; corners on both sides of it"""
    lo, hi = _box(camera_inside())
    assert (np.asarray(camera_inside().cam_pos) > lo).all() and (np.asarray(camera_inside().cam_pos) < hi).all()
    for make, sides in ((box_behind, {-1}), (box_straddles, {-1, 1})):
        r = make()
        lo, hi = _box(r)
        corners = np.array([[(lo, hi)[(k >> a) & 1][a] for a in range(3)] for k in range(8)])
        depth = (corners - np.asarray(r.cam_pos, np.float64)) @ np.asarray(r.cam_dir, np.float64)
        assert set(np.sign(depth).astype(int)) == sides


def test_a_tile_subset_splits_in_its_own_order():
    r = c2(80, 48)
    ids = np.array([14, 0, 7, 4, 9, 10], np.int32)
    clear = hk_sky.classify(r, ids)
    march, sky = hk_sky.split(r, ids)
    assert np.array_equal(march, ids[~clear]) and np.array_equal(sky, ids[clear]) and 0 < sky.size < ids.size


@pytest.mark.parametrize("name", SMALL)
def test_the_oracle_counts_only_primary_misses_in_clear_tiles(name):
    r = VIEWS[name][0]()
    clear = np.flatnonzero(hk_sky.classify(r))
    nx, _ = hk_sky.tiles_of(r.w, r.h)
    spp = 8
    for t in clear:
        x0, y0 = (t % nx) * 16, (t // nx) * 16
        rect = (x0, y0, min(x0 + 16, r.w), min(y0 + 16, r.h))
        o = VIEWS[name][0]()
        o.render(spp, rect=rect)
        c = o.counters.as_dict()
        assert c["n_primary_miss"] == spp * (rect[2] - rect[0]) * (rect[3] - rect[1]), (name, t, c)


@pytest.mark.parametrize("size", [(80, 48), (72, 56)])
@pytest.mark.parametrize("show_environment", [True, False])
def test_sky_sample_is_the_oracles_sample_bit_for_bit(size, show_environment):
    r = c2(*size)
    r.show_environment = show_environment
    clear = np.flatnonzero(hk_sky.classify(r))
    nx, _ = hk_sky.tiles_of(r.w, r.h)
    rng = np.random.default_rng(7)
    items = []
    for t in clear:
        x0, y0 = (t % nx) * 16, (t // nx) * 16
        for _ in range(60):
            items.append((rng.integers(x0, min(x0 + 16, r.w)), rng.integers(y0, min(y0 + 16, r.h)), rng.integers(1, 2000)))
    # the frame's lower right corner, which lies in a clear tile at both sizes, at the first samples
    assert nx - 1 in clear
    items += [(r.w - 1, 0, 1), (r.w - 1, 0, 2), (r.w - 2, 1, 3)]
    items = np.array(items, np.int32)
    assert items.shape[0] >= 200
    got, miss = hk_sky.samples(r, items)
    assert miss.all()
    want = np.stack([r.trace_pixel_sample(int(x), int(y), int(s)) for x, y, s in items])
    assert same(got, want)
    assert (want[:, 3] == 0).all() and (want[:, :3] > 0).any() == show_environment


def test_sky_sample_reports_a_ray_that_hits_and_produces_nothing():
    r = c2(80, 48)
    got, miss = hk_sky.samples(r, np.array([(40, 24, 1), (41, 25, 5)], np.int32))       # the frame's centre looks at the box
    assert not miss.any() and (got == -1.0).all()
