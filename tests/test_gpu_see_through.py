"""GPU: see-through tiles rendered outside the path scheduler (vr_set_int "see_through_tiles", vr_launch.hip sky_kernel without its box test, vr_sky_tiles.h).
A frame with the class on is the frame with it off and the oracle's, bit for bit -- whole frames, trace() loops, several sub-launches, a rank's share, moments,
adaptive sampling, no environment, poisoned pool and workspace, a dense fp16 grid -- and "last_see_through_tiles" says that the path under test ran, with the
count of the host build (tests/hk_see_through.py).  Off behind a transfer function, with an emission grid, in the tolerance mode and with the instrumented kernels."""
import numpy as np
import pytest

import hk_see_through as st
import scenes
from hk_common import bits as _bits

pytestmark = pytest.mark.gpu

SPP = 8
# W, H, clear tiles, see-through tiles of c2 (tests/test_see_through_host.py pins the same counts on the host build)
FRAMES = ((72, 56, 4, 1), (128, 128, 16, 7), (256, 256, 64, 56))
_ORACLE = {}


def oracle_frame(name, w, h, spp, show_environment=None):
    """show_environment None: as the scene's configuration leaves it"""
    key = (name, w, h, spp, show_environment)
    if key not in _ORACLE:
        o = scenes.oracle_scene(name, w, h)
        if show_environment is not None:
            o.show_environment = show_environment
        o.render(spp)
        o.fb.setflags(write=False)
        _ORACLE[key] = o.fb
    return _ORACLE[key]


def hip(name, w, h, see, **fields):
    r = scenes.hip_scene(name, w, h)
    r.see_through_tiles = see
    for k, v in fields.items():
        setattr(r, k, v)
    return r


def host_counts(name, w, h, tiles=None):
    cls, _ = st.classify(scenes.oracle_scene(name, w, h), tiles)
    return int((cls == st.CLEAR).sum()), int((cls == st.SEE).sum())


@pytest.mark.parametrize("w,h,n_clear,n_see", FRAMES)
def test_a_frame_with_the_class_is_the_frame_without_it_and_the_oracles(w, h, n_clear, n_see):
    assert host_counts("c2", w, h) == (n_clear, n_see)
    frames = {}
    for see in (1, 0):
        r = hip("c2", w, h, see)
        r.render(SPP)
        frames[see] = r.framebuffer()
        assert (r.last_see_through_tiles, r.last_sky_tiles, r.last_launches) == (n_see if see else 0, n_clear, 1)
        assert r.last_kernel_ms() > 0 and 0 < r.last_pathtrace_ms() <= r.last_kernel_ms()
        r.close()
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1]), _bits(oracle_frame("c2", w, h, SPP)))


def _trace_loop(r):
    for _ in range(SPP):
        r.trace()
    r.synchronize()


def _two_calls(r):
    r.render(3)
    r.render(SPP - 3)


def _one_call(r):
    r.render(SPP)


@pytest.mark.parametrize("how,fields,show", [(_trace_loop, {}, None), (_two_calls, {}, None), (_one_call, dict(order_tiles=2), None), (_one_call, dict(seed_table_mb=0), None),
                                             (_one_call, {}, False)],
                         ids=["trace_loop", "two_calls", "order_tiles_2", "hashed_seeds", "show_environment_0"])
@pytest.mark.parametrize("w,h,n_clear,n_see", FRAMES[:2])
def test_the_same_frame_however_it_is_submitted(how, fields, show, w, h, n_clear, n_see):
    frames = {}
    for see in (1, 0):
        r = hip("c2", w, h, see, **fields, **({} if show is None else dict(show_environment=show)))
        how(r)
        frames[see] = r.framebuffer()
        assert (r.last_see_through_tiles, r.last_sky_tiles, r.sample) == (n_see if see else 0, n_clear, SPP)
        r.close()
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1]), _bits(oracle_frame("c2", w, h, SPP, show)))
    if show is False:
        assert not frames[1][..., :3][frames[1][..., 3] == 0].any()


def test_several_sub_launches_of_a_small_pool():
    """16 MB hold 256 samples of the frame's twenty tiles at most: 1000 spp are several sub-launches, as many with the class as without it, each followed by the
    sky kernel over its sample window"""
    w, h, spp, frames, launches = 72, 56, 1000, {}, {}
    for see in (1, 0):
        r = hip("c2", w, h, see, sample_pool_mb=16)
        r.render(spp)
        frames[see] = r.framebuffer()
        launches[see] = r.last_launches
        assert (r.last_see_through_tiles, r.last_sky_tiles) == (1 if see else 0, 4)
        r.close()
    assert launches[1] == launches[0] and launches[1] > 1
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1]), _bits(oracle_frame("c2", w, h, spp)))


def _tile_pixels(ids, w, h):
    m = np.zeros((h, w), bool)
    nx = (w + 15) // 16
    for t in ids:
        m[(t // nx) * 16:(t // nx) * 16 + 16, (t % nx) * 16:(t % nx) * 16 + 16] = True
    return m


def test_a_ranks_share():
    from volren_amd.shard import TileShard
    w, h = 128, 128
    sh = TileShard(w, h, 2, 1)
    n_clear, n_see = host_counts("c2", w, h, sh.mine)
    assert 0 < n_see < 7 and 0 < n_clear
    frames = {}
    for see in (1, 0):
        r = hip("c2", w, h, see)
        r.set_tiles(sh.mine)
        r.render(SPP)
        frames[see] = r.framebuffer()
        assert (r.last_see_through_tiles, r.last_sky_tiles) == (n_see if see else 0, n_clear)
        r.close()
    mine = _tile_pixels(sh.mine, w, h)
    assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
    assert np.array_equal(_bits(frames[1][mine]), _bits(oracle_frame("c2", w, h, SPP)[mine])) and not frames[1][~mine].any()


@pytest.mark.parametrize("w,h,n_clear,n_see", FRAMES[:2])
def test_moments_are_the_same_too(w, h, n_clear, n_see):
    got = {}
    for see in (1, 0):
        r = hip("c2", w, h, see, variance=1)
        r.render(3)
        r.render(SPP - 3)
        got[see] = (r.framebuffer(), r.variance())
        assert r.last_see_through_tiles == (n_see if see else 0)
        r.close()
    assert np.array_equal(_bits(got[1][0]), _bits(got[0][0])) and np.array_equal(_bits(got[1][1]), _bits(got[0][1]))
    assert np.array_equal(_bits(got[1][0]), _bits(oracle_frame("c2", w, h, SPP)))


def test_adaptive_sampling_with_and_without_the_class():
    w, h = 72, 56
    base = hip("c2", w, h, 0, variance=1)
    base.render(8)
    thr = float(np.median(base.tile_error()[np.isfinite(base.tile_error())]))
    base.close()
    got = {}
    for see in (1, 0):
        r = hip("c2", w, h, see)
        r.render_adaptive(2, 8, thr)
        got[see] = (r.framebuffer(), r.variance(), r.tile_samples(), r.adaptive_rounds)
        r.close()
    assert len(set(got[0][2].reshape(-1).tolist())) >= 2                       # the threshold spreads the counts: groups of several sizes ran
    for a, b in zip(got[1][:3], got[0][:3]):
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
    assert got[1][3] == got[0][3]


def test_poisoned_workspace_and_pool_change_nothing(monkeypatch):
    monkeypatch.setenv("VR_TEST_POISON_WORKSPACE", "2")
    for w, h, n_clear, n_see in FRAMES[:2]:
        r = hip("c2", w, h, 1)
        r.render(3)
        r.render(SPP - 3)
        assert (r.last_see_through_tiles, r.last_sky_tiles) == (n_see, n_clear)
        assert np.array_equal(_bits(r.framebuffer()), _bits(oracle_frame("c2", w, h, SPP)))
        r.close()


def test_a_dense_fp16_grid_with_empty_coarse_cells():
    """the range table of a DenseGridF16, and rays that enter the box through cells whose majorant is 0 on the coarsest level"""
    import encoder_ref
    vox = np.zeros((128, 128, 128), np.float16)
    vox[0:8, 0:8, 0:8] = np.float16(5.0)
    w = h = 128
    o = scenes.oracle_scene("c2", w, h)
    o.set_volume(encoder_ref.encode_dense_fp16(vox))
    cls, _ = st.classify(o)
    n_clear, n_see = int((cls == st.CLEAR).sum()), int((cls == st.SEE).sum())
    assert n_see >= 8
    want = o.render(SPP)
    frames = {}
    for see in (1, 0):
        r = hip("c2", w, h, see)
        r.set_volume_dense_f16(vox)
        r.render(SPP)
        frames[see] = r.framebuffer()
        assert (r.last_see_through_tiles, r.last_sky_tiles) == (n_see if see else 0, n_clear)
        r.close()
    assert np.array_equal(_bits(frames[1]), _bits(frames[0])) and np.array_equal(_bits(frames[1]), _bits(want))


def test_no_see_through_tile_behind_a_lut_or_with_an_emission_grid():
    """c3: a transfer function; c5: an emission grid (and float grids, encoded on the device: the host holds no range table); c4: a dense fp16 grid filled throughout,
    which has as many see-through tiles as the host build says"""
    for name, w, h in (("c3", 128, 128), ("c5:64", 80, 48), ("c4:64", 80, 48)):
        frames = {}
        n_see = host_counts(name, w, h)[1] if name == "c4:64" else 0
        for see in (1, 0):
            r = hip(name, w, h, see)
            r.render(4)
            frames[see] = r.framebuffer()
            assert r.last_see_through_tiles == (n_see if see else 0)
            r.close()
        assert np.array_equal(_bits(frames[1]), _bits(frames[0]))
        if name == "c3":
            assert np.array_equal(_bits(frames[1]), _bits(oracle_frame("c3", w, h, 4)))


def test_the_class_is_off_where_the_split_is_off_and_for_the_other_integrators():
    r = hip("c2", 128, 128, 1)
    r.render(2)
    assert (r.last_see_through_tiles, r.last_sky_tiles) == (7, 16)
    r.sched_stats(True)
    r.render(2)
    assert (r.last_see_through_tiles, r.last_sky_tiles) == (0, 0)
    r.sched_stats(False)
    r.fast_math = 1
    r.render(2)
    assert (r.last_see_through_tiles, r.last_sky_tiles) == (0, 0)
    r.fast_math = 0
    r.render(2)
    assert (r.last_see_through_tiles, r.last_sky_tiles) == (7, 16) and r.sample == 8
    r.integrator = 1                                   # the global-majorant tracker: the class holds for it
    r.render(2)
    assert (r.last_see_through_tiles, r.last_sky_tiles) == (7, 16)
    r.sky_tiles = 0                                    # effective only where the clear tiles are split off
    r.render(2)
    assert (r.last_see_through_tiles, r.last_sky_tiles) == (0, 0) and np.isfinite(r.framebuffer()).all()
    r.close()


def test_integrator_1_with_the_class_is_the_oracles_frame():
    w, h = 72, 56
    o = scenes.oracle_scene("c2", w, h)
    o.integrator = 1
    want = o.render(SPP)
    r = hip("c2", w, h, 1, integrator=1)
    r.render(SPP)
    assert r.last_see_through_tiles == 1
    assert np.array_equal(_bits(r.framebuffer()), _bits(want))
    r.close()
