"""GPU: the temporal luminance moments (vr_set_int "denoise_moments", vr_denoise_history_moments) through the C ABI: the temporal and the variance
kernel equal the host-compiled lane code bit for bit (tests/hostkernel/moments_host.cpp, itself held to a float64 statement by
tests/test_moments_host.py) on sequences with a fixed and a turning camera and on degenerate frames; the values of the setting; a change drops the
history; the refusal together with rejection; logical shards; and what it is for: frames of 1 spp are filtered."""
import numpy as np
import pytest

import hk_moments as hm
import scenes
import volren_amd
from gpu_frames import _camera, _frame, _orbit, _scene
from hk_common import bits as _bits
from hk_common import same as _same
from test_moments_capi import check_values
from test_moments_host import FRAMES, H4, W4, check_low_spp, run_low_spp

pytestmark = pytest.mark.gpu


def _moments_scene(name, w, h):
    r = _scene(name, w, h)
    r.denoise_moments = 1
    return r


def _check(r, replay, what):
    """after r.denoise_temporal(): history, moment records and result equal the host lane code fed with the renderer's own buffers and camera -> N"""
    hc, hv, hn = r.denoise_history()
    want = replay.frame(_camera(r), r.framebuffer(), r.variance(), r.features(), r.sample, r.denoise_alpha, r.denoise_iterations, tuple(r.denoise_sigma))
    for got, ref, part in ((hc, want[0], "C"), (hv, want[1], "V"), (hn, want[2], "N"), (r.denoise_history_moments(), want[3], "moments"), (r.denoised(), want[4], "denoised")):
        bad = _bits(got) != _bits(ref)
        assert not bad.any(), (what, part, int(bad.sum()))
    return hn


# ---- 1: the kernels are the host lane code, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spp,iterations", (("c2", 1, 5), ("c2", 3, 5), ("c3", 1, 5), ("c2", 1, 0)))
def test_fixed_then_turning_camera_matches_the_host_lane_code(name, spp, iterations):
    """40 x 24: 3 x 2 tiles, both edges ragged, the 3-pixel halo crosses tile and frame edges.  Four frames under a fixed camera, then 1 degree per
    frame about the volume for three: reprojection, disoccluded pixels with N < 4 and pixels with N >= 4 side by side."""
    r = _moments_scene(name, 40, 24)
    r.denoise_iterations = iterations
    replay = hm.Replay()
    for i in range(7):
        _orbit(r, 1.0 * max(0, i - 3))
        _frame(r, spp, seed=i + 1)
        r.denoise_temporal()
        n = _check(r, replay, (name, spp, i))
        if i == 0:
            assert (n == 1).all()
    assert (n < 4).any() and (n >= 4).any(), np.bincount(n.astype(int).reshape(-1))


# one pixel, less than a wave, one pixel in each second tile, exactly one tile; thin both ways, one pixel past a tile, one short of two tiles: the
# staged window's halo of 3 leaves the frame on each side in turn and crosses a tile edge with a partial tile next to it
@pytest.mark.parametrize("w,h", ((1, 1), (2, 3), (17, 17), (16, 16), (1, 37), (37, 1), (17, 16), (33, 31)))
def test_degenerate_frames(w, h):
    r = _moments_scene("c2", w, h)
    replay = hm.Replay()
    for i in range(2):
        _frame(r, 1, seed=i + 1)
        r.denoise_temporal()
        _check(r, replay, (w, h, i))


# ---- 2: the setting -------------------------------------------------------------------------------------------------------------------------------------
def test_the_values_of_the_setting():
    check_values(volren_amd.Renderer(16, 16))


def test_a_change_of_the_setting_drops_the_history_and_zero_has_no_moment_records():
    r = _scene("c2", 24, 16)
    _frame(r, 2, seed=1)
    r.denoise_temporal()
    r.denoise_history()
    with pytest.raises(volren_amd.VolrenError, match="denoise_history_moments"):
        r.denoise_history_moments()                   # the setting is 0: a history without moment records
    r.denoise_moments = 0                             # no change: the history stays
    r.denoise_history()
    r.denoise_moments = 1
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 1).all() and r.denoise_history_moments().shape == (16, 24, 4)
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 2).all()
    r.denoise_moments = 0
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    with pytest.raises(volren_amd.VolrenError, match="denoise_history_moments"):
        r.denoise_history_moments()
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 1).all()


def test_moments_and_rejection_together_are_refused_and_change_nothing():
    r = _moments_scene("c2", 24, 16)
    for i in range(2):
        _frame(r, 2, seed=i + 1, fseed=7)           # (one guide for every frame: no tap rule restarts a pixel)
        r.denoise_temporal()
    before, records, result = r.denoise_history(), r.denoise_history_moments(), r.denoised()
    _frame(r, 2, seed=3, fseed=7)
    r.denoise_reject = 3.0
    with pytest.raises(volren_amd.VolrenError, match="denoise_moments.*denoise_reject"):
        r.denoise_temporal()
    assert all(_same(a, b) for a, b in zip(before, r.denoise_history()))
    assert _same(records, r.denoise_history_moments()) and _same(result, r.denoised())
    r.denoise_reject = 0.0
    r.denoise_temporal()                              # and without it the sequence goes on
    assert (r.denoise_history()[2] == 3).all()


# ---- 3: shards --------------------------------------------------------------------------------------------------------------------------------------------
def test_two_logical_shards_equal_one_device():
    name, w, h = "c2", 48, 32
    one = _moments_scene(name, w, h)
    s = volren_amd.ShardedRenderer(w, h, [0, 0])
    s.each(lambda p: scenes.configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    s.parts[0].denoise_moments = 1                    # the filter's settings are part 0's
    assert s.denoise_moments == 1
    for frame in range(3):
        for r in (one, s):
            if r is one:
                r.seed = frame + 1
            else:
                def seed(p):
                    p.seed = frame + 1
                r.each(seed)
            r.reset()
            r.render(1)
            r.render_features(1)
            r.denoise_temporal()
        assert _same(s.denoised(), one.denoised()), frame
        for a, b in zip(s.denoise_history(), one.denoise_history()):
            assert _same(a, b), frame
        assert _same(s.denoise_history_moments(), one.denoise_history_moments()), frame
    one.close()
    s.close()


# ---- 4: what it is for --------------------------------------------------------------------------------------------------------------------------------------
def test_one_sample_per_pixel_is_filtered():
    """tests/test_moments_host.py's table and bounds through volren_amd.Renderer: c2 at 64x48, 16 frames of 1 spp, seeds 100 .. 115, fixed camera,
    against 1024 spp of seed 777.  The pipeline is bit-exact, so the numbers are the CPU test's."""
    ref = _scene("c2", W4, H4)
    ref.variance = 0
    ref.seed = 777
    ref.render(1024)

    def run_of(moments, iterations):
        r = _scene("c2", W4, H4)
        r.denoise_moments = moments
        r.denoise_iterations = iterations

        def one(cam, i):
            _frame(r, 1, seed=100 + i)
            r.denoise_temporal()
            return r.denoised()
        return one

    check_low_spp(run_low_spp(lambda i: i, ref.framebuffer(), None, lambda iterations: run_of(0, iterations), lambda: run_of(1, 5), frames=FRAMES))
