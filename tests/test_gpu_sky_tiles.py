"""GPU: clear tiles rendered outside the path scheduler (vr_set_int "sky_tiles", vr_launch.hip sky_kernel, vr_sky_tiles.h).  A frame with the split is the frame
without it and the oracle's, bit for bit -- whole frames, frames in several calls, trace() loops, several sub-launches, either tile order, a rank's share,
moments, adaptive sampling, a view of nothing but clear tiles -- and "last_sky_tiles" says that the path under test ran.  Off with the instrumented kernels
and in the tolerance mode."""
import numpy as np
import pytest

import hk_sky
import scenes
from hk_common import bits as _bits

pytestmark = pytest.mark.gpu

SPP = 8
# scene, W, H, clear tiles (tests/test_sky_tiles_host.py pins the same counts on the host build)
FRAMES = (("c2", 80, 48, 6), ("c2", 72, 56, 4), ("c3", 80, 48, 6), ("c4_64", 80, 48, 0))
_ORACLE = {}


def oracle_frame(name, w, h, spp, variant=None):
    key = (name, w, h, spp, variant)
    if key not in _ORACLE:
        o = scenes.oracle_scene(name, w, h)
        if variant == "away":
            _look_away(o)
        o.render(spp)
        o.fb.setflags(write=False)
        _ORACLE[key] = o.fb
    return _ORACLE[key]


def hip(name, w, h, sky, **fields):
    r = scenes.hip_scene(name, w, h)
    r.sky_tiles = sky
    for k, v in fields.items():
        setattr(r, k, v)
    return r


def _tile_pixels(ids, w, h):
    """[H][W] mask of the pixels of the listed raster tiles"""
    m = np.zeros((h, w), bool)
    nx = (w + 15) // 16
    for t in ids:
        m[(t // nx) * 16:(t // nx) * 16 + 16, (t % nx) * 16:(t % nx) * 16 + 16] = True
    return m


@pytest.mark.parametrize("name,w,h,n_clear", FRAMES)
def test_a_frame_with_the_split_is_the_frame_without_it_and_the_oracles(name, w, h, n_clear):
    frames = {}
    for sky in (1, 0):
        r = hip(name, w, h, sky)
        r.render(SPP)
        frames[sky] = r.framebuffer()
        assert r.last_sky_tiles == (n_clear if sky else 0) and r.last_launches == 1
        assert r.last_kernel_ms() > 0 and 0 < r.last_pathtrace_ms() <= r.last_kernel_ms()
        r.close()
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1]), _bits(oracle_frame(name, w, h, SPP)))


def _two_calls(r):
    r.render(3)
    r.render(SPP - 3)


def _trace_loop(r):
    for _ in range(SPP):
        r.trace()
    r.synchronize()


def _one_call(r):
    r.render(SPP)


@pytest.mark.parametrize("how,fields", [(_two_calls, {}), (_trace_loop, {}), (_one_call, dict(order_tiles=0)), (_one_call, dict(order_tiles=2)), (_one_call, dict(seed_table_mb=0))],
                         ids=["two_calls", "trace_loop", "order_tiles_0", "order_tiles_2", "hashed_seeds"])
@pytest.mark.parametrize("w,h,n_clear", [(80, 48, 6), (72, 56, 4)])
def test_the_same_frame_however_it_is_submitted(how, fields, w, h, n_clear):
    frames = {}
    for sky in (1, 0):
        r = hip("c2", w, h, sky, **fields)
        how(r)
        frames[sky] = r.framebuffer()
        assert r.last_sky_tiles == (n_clear if sky else 0) and r.sample == SPP
        r.close()
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1]), _bits(oracle_frame("c2", w, h, SPP)))


def test_several_sub_launches_of_a_small_pool():
    """16 MB hold 256 samples of the frame's fifteen tiles: 1000 spp are four sub-launches with the split as without it, each followed by the sky kernel
    over its sample window"""
    spp, frames = 1000, {}
    for sky in (1, 0):
        r = hip("c2", 80, 48, sky, sample_pool_mb=16)
        r.render(spp)
        frames[sky] = r.framebuffer()
        assert (r.last_sky_tiles, r.last_launches) == ((6, 4) if sky else (0, 4))
        r.close()
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1]), _bits(oracle_frame("c2", 80, 48, spp)))


def test_a_ranks_share():
    from volren_amd.shard import TileShard
    w, h = 80, 48
    sh = TileShard(w, h, 2, 1)
    o = scenes.oracle_scene("c2", w, h)
    clear = hk_sky.classify(o, sh.mine)
    assert 0 < clear.sum() < len(sh.mine)
    frames = {}
    for sky in (1, 0):
        r = hip("c2", w, h, sky)
        r.set_tiles(sh.mine)
        r.render(SPP)
        frames[sky] = r.framebuffer()
        assert r.last_sky_tiles == (int(clear.sum()) if sky else 0)
        r.close()
    mine = _tile_pixels(sh.mine, w, h)
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1][mine]), _bits(oracle_frame("c2", w, h, SPP)[mine])) and not frames[1][~mine].any()


@pytest.mark.parametrize("w,h,n_clear", [(80, 48, 6), (72, 56, 4)])
def test_moments_are_the_same_too(w, h, n_clear):
    got = {}
    for sky in (1, 0):
        r = hip("c2", w, h, sky, variance=1)
        r.render(3)
        r.render(SPP - 3)
        got[sky] = (r.framebuffer(), r.variance())
        assert r.last_sky_tiles == (n_clear if sky else 0)
        r.close()
    assert np.array_equal(_bits(got[1][0]), _bits(got[0][0])) and np.array_equal(_bits(got[1][1]), _bits(got[0][1]))
    assert np.array_equal(_bits(got[1][0]), _bits(oracle_frame("c2", w, h, SPP)))
    clear = _tile_pixels(np.flatnonzero(hk_sky.classify(scenes.oracle_scene("c2", w, h))), w, h)
    assert (got[1][1][clear][:, 3] == 0).all() and (got[1][1][clear][:, :3] > 0).any()        # alpha never varies there; the jittered environment does


def test_adaptive_sampling_with_and_without_the_split():
    w, h = 72, 56
    base = hip("c2", w, h, 0, variance=1)
    base.render(8)
    thr = float(np.median(base.tile_error()[np.isfinite(base.tile_error())]))
    base.close()
    got = {}
    for sky in (1, 0):
        r = hip("c2", w, h, sky)
        r.render_adaptive(2, 8, thr)
        got[sky] = (r.framebuffer(), r.variance(), r.tile_samples(), r.adaptive_rounds)
        r.close()
    assert len(set(got[0][2].reshape(-1).tolist())) >= 2                       # the threshold spreads the counts: groups of several sizes ran
    for a, b in zip(got[1][:3], got[0][:3]):
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
    assert got[1][3] == got[0][3]


def _look_away(r):
    """from further off and pitched up by 45 degrees: the box lies in front of the camera plane and below the frame"""
    r.cam_pos = (3.0, 0.0, 3.0)
    r.cam_dir = (-0.5, float(np.sqrt(0.5)), -0.5)


def test_a_view_of_nothing_but_clear_tiles_launches_no_path_tracer():
    w, h = 80, 48
    o = scenes.oracle_scene("c2", w, h)
    _look_away(o)
    assert hk_sky.classify(o).all()
    r = hip("c2", w, h, 1, variance=1)
    _look_away(r)
    r.render(3)
    assert (r.last_sky_tiles, r.last_launches) == (15, 0)
    r.render(SPP - 3)
    assert (r.last_sky_tiles, r.last_launches) == (15, 0) and r.last_kernel_ms() > 0
    fb = r.framebuffer()
    assert np.array_equal(_bits(fb), _bits(oracle_frame("c2", w, h, SPP, "away"))) and (fb[..., 3] == 0).all() and (fb[..., :3] > 0).all()
    r.sky_tiles = 0
    r.reset()
    r.render(SPP)
    assert (r.last_sky_tiles, r.last_launches) == (0, 1) and np.array_equal(_bits(r.framebuffer()), _bits(fb))
    r.close()


def test_the_split_is_off_for_the_instrumented_kernels_and_the_tolerance_mode():
    r = hip("c2", 80, 48, 1)
    r.render(2)
    assert r.last_sky_tiles == 6
    r.sched_stats(True)
    r.render(2)
    assert r.last_sky_tiles == 0
    r.sched_stats(False)
    r.fast_math = 1
    r.render(2)
    assert r.last_sky_tiles == 0
    r.fast_math = 0
    r.render(2)
    assert r.last_sky_tiles == 6 and r.sample == 8
    r.integrator = 3
    r.render(2)
    assert r.last_sky_tiles == 0 and np.isfinite(r.framebuffer()).all()
    r.close()


def test_poisoned_workspace_and_pool_change_nothing(monkeypatch):
    monkeypatch.setenv("VR_TEST_POISON_WORKSPACE", "2")
    for w, h, n_clear in ((80, 48, 6), (72, 56, 4)):
        r = hip("c2", w, h, 1)
        r.render(3)
        r.render(SPP - 3)
        assert r.last_sky_tiles == n_clear
        assert np.array_equal(_bits(r.framebuffer()), _bits(oracle_frame("c2", w, h, SPP)))
        r.close()
