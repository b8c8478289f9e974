"""Denoising on the sharded renderer (include/volren_amd.h vr_sharded_render_features / _gather_guides / _denoise / _denoise_temporal,
volren_amd/csrc/sharded.h): every part computes the moments and features of its own tiles, ONE exchange takes them to part 0, part 0 filters
the whole frame -- bit for bit what a single device gives, NaN patterns included (everything is compared as uint32).

The parts are logical shards of device 0 (device-to-device copies ordered by events stand in for the collective), and RCCL carries one rank,
as in test_gpu_sharded.py: the guide exchange has never run between two physical devices."""
import numpy as np
import pytest

from hk_common import same as _same
import scenes

pytestmark = pytest.mark.gpu


_REF = {}


def _reference(name, w, h, spp, fspp, iterations=None):
    """the single-device run every test compares with: variance = 1, render, render_features, denoise.  Computed once per key, never changed"""
    key = (name, w, h, spp, fspp, iterations)
    if key not in _REF:
        r = scenes.hip_scene(name, w, h)
        r.variance = 1
        if iterations is not None:
            r.denoise_iterations = iterations
        r.render(spp)
        r.render_features(fspp)
        r.denoise()
        _REF[key] = dict(frame=r.framebuffer(), variance=r.variance(), features=r.features(), denoised=r.denoised())
        for a in _REF[key].values():
            a.setflags(write=False)
        r.close()
    return _REF[key]


def _sharded(name, w, h, devices):
    import volren_amd
    s = volren_amd.ShardedRenderer(w, h, devices)
    s.each(lambda p: scenes.configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    return s


def _check(s, ref):
    assert _same(s.denoised(), ref["denoised"])
    assert _same(s.variance(), ref["variance"])
    assert _same(s.features(), ref["features"])
    assert _same(s.framebuffer(), ref["frame"])            # still the plain frame


# a transfer function (c3), partial tiles with unequal tile counts per part (150x90 / 3, 70x52 / 5), parts that own no tile (32x32 / 8, 16x16 / 2)
@pytest.mark.parametrize("name,w,h,spp,fspp,parts", [("c1", 150, 90, 3, 2, 3), ("c3", 96, 64, 4, 3, 2), ("c2", 70, 52, 5, 4, 5), ("c1", 32, 32, 3, 2, 8),
                                                     ("c1", 16, 16, 2, 2, 2)])
def test_logical_shards_equal_the_single_device_result(name, w, h, spp, fspp, parts):
    ref = _reference(name, w, h, spp, fspp)
    s = _sharded(name, w, h, [0] * parts)
    assert s.transport == "copy" and len(s.parts) == parts
    s.render(spp)
    s.render_features(fspp)
    s.denoise()
    _check(s, ref)
    s.close()


@pytest.mark.parametrize("iterations", (0, 1))
def test_copy_only_and_single_iteration_paths(iterations):
    name, w, h, spp, fspp, parts = "c1", 150, 90, 3, 2, 3
    ref = _reference(name, w, h, spp, fspp, iterations)
    s = _sharded(name, w, h, [0] * parts)
    s.parts[0].denoise_iterations = iterations             # the filter's settings are part 0's
    s.render(spp)
    s.render_features(fspp)
    s.denoise()
    _check(s, ref)
    if iterations == 0:
        assert _same(s.denoised(), ref["frame"])
    s.close()


def test_frames_back_to_back_without_synchronisation():
    name, w, h, spp, fspp, parts = "c1", 150, 90, 3, 2, 3
    ref = _reference(name, w, h, spp, fspp)
    s = _sharded(name, w, h, [0] * parts)
    for _ in range(2):
        s.reset()
        s.render(spp, sync=False)
        s.render_features(fspp, sync=False)
        s.denoise(sync=False)
    s.reset()                                              # ... and a frame accumulated in two calls
    s.render(spp - 1, sync=False)
    s.render(1, sync=False)
    s.render_features(fspp, sync=False)
    s.denoise(sync=False)
    s.synchronize()
    _check(s, ref)
    s.close()


def _orbit(r, degrees):
    """not gpu_frames._orbit(r, degrees, 0.0): cam_dir.y is -0.0 here and +0.0 there"""
    a = np.radians(45.0 + degrees)
    pos = np.array([np.sqrt(2.0) * np.sin(a), 0.0, np.sqrt(2.0) * np.cos(a)])
    r.cam_pos = pos
    r.cam_dir = -pos / np.linalg.norm(pos)


def test_temporal_sequence_equals_the_single_device_sequence():
    name, w, h, spp, fspp, parts = "c2", 70, 52, 3, 2, 3
    one = scenes.hip_scene(name, w, h)
    one.variance = 1
    s = _sharded(name, w, h, [0] * parts)
    for frame in range(3):
        if frame == 2:                                     # the camera turns between frames 2 and 3: the history is reprojected
            _orbit(one, 3.0)
            s.each(lambda p: _orbit(p, 3.0))
        for r in (one, s):
            r.reset()
            r.render(spp)
            r.render_features(fspp)
            r.denoise_temporal()
        assert _same(s.denoised(), one.denoised()), frame
        for a, b in zip(s.denoise_history(), one.denoise_history()):
            assert _same(a, b), frame
    s.denoise_history_reset()
    one.denoise()
    s.denoise_temporal()                                   # no history: what denoise() gives
    assert _same(s.denoised(), one.denoised())
    s.denoise()
    assert _same(s.denoised(), one.denoised())
    one.close()
    s.close()


def test_refusals_leave_the_result_and_the_object_usable():
    import volren_amd
    name, w, h, spp, fspp, parts = "c1", 70, 52, 3, 2, 3
    ref = _reference(name, w, h, spp, fspp)
    s = _sharded(name, w, h, [0] * parts)
    s.render(spp)
    with pytest.raises(volren_amd.VolrenError, match="render_features"):       # no feature pass yet
        s.denoise()
    with pytest.raises(volren_amd.VolrenError):
        s.gather_guides()
    s.render_features(fspp)
    s.denoise_temporal()
    _check(s, ref)
    history = s.denoise_history()
    # variance off on part 1 only
    s.reset()
    s.parts[1].variance = 0
    s.render(spp)
    s.render_features(fspp)
    for call in (s.denoise, s.denoise_temporal):
        with pytest.raises(volren_amd.VolrenError, match="part 1"):
            call()
    s.parts[1].variance = 1
    assert _same(s.denoised(), ref["denoised"])
    # sample = 0
    s.reset()
    for call in (s.denoise, s.denoise_temporal):
        with pytest.raises(volren_amd.VolrenError, match="sample < 1"):
            call()
    assert _same(s.denoised(), ref["denoised"])
    for a, b in zip(s.denoise_history(), history):
        assert _same(a, b)
    # a correct sequence afterwards
    s.render(spp)
    s.render_features(fspp)
    s.denoise()
    _check(s, ref)
    with pytest.raises(volren_amd.VolrenError, match="tile subset"):           # a part on its own still refuses
        s.parts[0].denoise()
    assert _same(s.denoised(), ref["denoised"])
    s.close()


def test_one_part_is_the_plain_renderer_and_rccl_carries_one_rank(monkeypatch):
    name, w, h, spp, fspp = "c1", 96, 64, 4, 3
    ref = _reference(name, w, h, spp, fspp)
    s = _sharded(name, w, h, [0])
    assert s.transport == "none"
    s.render(spp)
    s.render_features(fspp)
    s.denoise()
    _check(s, ref)
    s.close()
    monkeypatch.setenv("VR_SHARDED_TRANSPORT", "rccl")
    for collective in ("gather", "allgather"):
        monkeypatch.setenv("VR_SHARDED_COLLECTIVE", collective)
        s = _sharded(name, w, h, [0])
        assert s.transport == "rccl" and s.collective == collective
        s.render(spp)
        s.render_features(fspp)
        s.denoise()
        _check(s, ref)
        s.reset(); s.render(spp); s.render_features(fspp); s.denoise_temporal()       # the second exchange through the same buffers
        _check(s, ref)
        s.close()
