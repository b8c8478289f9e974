"""GPU: the hot pair's collision block evaluates what the path's state alone determines before it waits for the tap (vr_trace.h collide_finish EARLY,
vr_pathtrace.h collide_tail_early) -- a change of order only, so every frame below must still be the oracle's, bit for bit.

Frames of 72 x 56: ragged against the 8 x 8 tiles and against the work units.  The scenes of every kernel variant; a white medium with 1000 bounces, where
most shadow rays end blocked (the shortcut's side of the collision), from the scene's camera (the clean copies of the hot pair) and from very far away (the
general copy); collide thresholds 1 and 64, so that lanes wait at a tentative collision across event batches; a small environment map in compact and in float
form, whose lookups cross the seam; and the tolerance-mode kernels, held to their bound of 1e-3 relative L2."""
import functools

import numpy as np
import pytest

import scenes
from test_gpu_parity import FLAG_VARIANTS, _assert_same, _bits

pytestmark = pytest.mark.gpu

W, H = 72, 56


def _white(x):
    x.albedo, x.bounces = (1.0, 1.0, 1.0), 1000


def _far(x):
    for k, v in FLAG_VARIANTS["camera_very_far"][1].items():
        setattr(x, k, v)


def _small_env(exact_rgbe):
    """a 5 x 4 map of exact RGBE texels (test_small_environment_maps_in_compact_form); one texel nudged off that grid keeps the whole map in float form"""
    w, h = 5, 4
    rs = np.random.RandomState(w * 100 + h)
    m = rs.randint(0, 256, (h, w, 3)).astype(np.float32)
    m[..., 0] = rs.randint(128, 256, (h, w))
    m[..., 1:] = np.minimum(m[..., 1:], m[..., :1])
    env = (m * np.exp2(rs.randint(-12, 2, (h, w, 1)).astype(np.float32))).astype(np.float32)
    env[0, 0] = 0.0
    if not exact_rgbe:
        env[h - 1, w - 1, 1] = np.float32(1.0 / 3.0)
    return env


SETUPS = {
    "plain": lambda x: None,
    "white": _white,
    "white_far": lambda x: (_white(x), _far(x)),
    "env_compact": lambda x: x.set_envmap(_small_env(True)),
    "env_float": lambda x: x.set_envmap(_small_env(False)),
}


@functools.lru_cache(maxsize=None)
def _oracle(name, setup, spp):
    o = scenes.oracle_scene(name, W, H)
    SETUPS[setup](o)
    f = o.render(spp).copy()
    f.setflags(write=False)
    return f


def _hip(name, setup):
    r = scenes.hip_scene(name, W, H)
    SETUPS[setup](r)
    return r


@pytest.mark.parametrize("name", ["c2", "c3", "c4:64", "c5:64"])
def test_every_scene_kind(name):
    r = _hip(name, "plain")
    r.render(24)
    _assert_same(r.framebuffer(), _oracle(name, "plain", 24), name)


@pytest.mark.parametrize("setup", ["white", "white_far"])
def test_white_medium_of_1000_bounces(setup):
    r = _hip("c2", setup)
    r.render(6)
    _assert_same(r.framebuffer(), _oracle("c2", setup, 6), setup)


@pytest.mark.parametrize("thr", [1, 64])
@pytest.mark.parametrize("setup", ["plain", "white"])
def test_lanes_waiting_at_a_collision(setup, thr):
    spp = 24 if setup == "plain" else 6
    r = _hip("c2", setup)
    r.set_sched([64, 0, 56, thr, 60, 60, 64, 0])        # NEW, pool cap, hungry, collide threshold, NEE, POSTNEE, ESCAPE
    r.render(spp)
    _assert_same(r.framebuffer(), _oracle("c2", setup, spp), "%s, collide threshold %d" % (setup, thr))


@pytest.mark.parametrize("setup, compact", [("env_compact", 1), ("env_float", 0)])
def test_small_environment_map(setup, compact):
    r = _hip("c2", setup)
    assert r.env_compact == compact
    r.render(24)
    _assert_same(r.framebuffer(), _oracle("c2", setup, 24), setup)


def test_tolerance_mode_stays_within_its_bound():
    """The tolerance-mode kernels are not the oracle's arithmetic: their frame is held to 1e-3 relative L2 at 1024 spp, where the figure is about the renderer and
    not about one flipped path (test_hip_within_1e3_of_reference_glsl_at_1024_spp).  The reference here is the bit-exact kernels' frame of the same samples -- the
    oracle's frame, as the tests above hold it at this size."""
    r = _hip("c2", "plain")
    r.render(24)
    _assert_same(r.framebuffer(), _oracle("c2", "plain", 24), "c2")
    r.reset(); r.render(1024)
    exact = r.framebuffer().copy()
    r.fast_math = 1
    r.reset(); r.render(1024)
    rl2 = scenes.rel_l2(r.framebuffer()[..., :3], exact[..., :3])
    print("tolerance mode, c2 %dx%d 1024 spp: relative L2 %.3e" % (W, H, rl2))
    assert rl2 <= 1e-3, rl2
