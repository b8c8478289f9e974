"""GPU: the history rejection of the temporal accumulation (vr_set_float "denoise_reject", vr_denoise_reject_stat) through the C ABI: the fetch and
resolve kernels equal the host-compiled lane code bit for bit (tests/hostkernel/temporal_host.cpp, itself held to a float64 statement by
tests/test_reject_host.py), statistic included; a threshold of 0 is the call as it was; the state rules; a scratch buffer that does not fit; logical
shards; that it follows a changing scene; the Python, volpy and CLI interfaces."""
import subprocess

import numpy as np
import pytest

import hk_adaptive
import hk_temporal as ht
import scenes
import volren_amd
from gpu_frames import _camera, _check_against_replay, _frame, _orbit, _scene
from hk_common import same as _same
from test_reject_capi import check_range
from test_reject_host import CHANGE, H3, SPP, W3, change_scene, check_table, run_scenarios

pytestmark = pytest.mark.gpu


def _sequence(r, tau, what, frames=4, spp=5):
    """an orbit of 1 degree steps with the density scaled by 0.25 in the middle; -> (pixels kept with N >= 2, pixels rejected) over the sequence"""
    r.denoise_reject = tau
    replay = ht.Replay()
    kept = dropped = 0
    for i in range(frames):
        _orbit(r, 1.0 * i)
        if i == frames // 2:
            r.density_scale = 0.25 * r.density_scale
        _frame(r, spp, seed=i + 1)
        r.denoise_temporal()
        n, stat = _check_against_replay(r, replay, (what, tau, i))
        kept += int((n >= 2).sum())
        dropped += int(ht.rejected(stat, tau).sum())
    return kept, dropped


# ---- 1: the kernels are the host lane code, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", (3.0, 0.5))
@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
def test_moving_sequence_with_a_change_matches_the_host_lane_code(name, tau):
    kept, dropped = _sequence(_scene(name, 33, 31), tau, name)
    print("%s tau %g: %d kept, %d rejected" % (name, tau, kept, dropped))
    assert kept + dropped > 0
    if name == "c1":
        assert kept > 0 and dropped > 0, (kept, dropped)      # both outcomes ran (c3's 5 spp frames are too noisy for its change to show at tau = 3)


# one tile, partial tiles, halos that cross tile edges and the frame's edges
@pytest.mark.parametrize("w,h", ((1, 1), (1, 37), (37, 1), (15, 9), (17, 16), (40, 36)))
def test_small_and_thin_frames(w, h):
    for tau in (3.0, 0.5):
        _sequence(_scene("c1", w, h), tau, (w, h), frames=3)


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_ragged_frame_as_the_second_frame():
    W, H = 64, 48
    r = _scene("c4_64", W, H)
    r.denoise_reject = 3.0
    replay = ht.Replay()
    _frame(r, 8, seed=1)
    r.denoise_temporal()
    _check_against_replay(r, replay, "uniform")
    _orbit(r, 2.0)
    r.seed = 2
    r.reset()
    r.render_adaptive(2, 8, 0.0)
    r.set_tiles([1, 2, 7])
    r.render_adaptive(2, 32, 0.0)
    r.set_tiles([])
    counts = r.tile_samples()
    assert sorted(set(counts.reshape(-1).tolist())) == [8, 32]
    r.render_features(8)
    r.denoise_temporal()
    n, stat = _check_against_replay(r, replay, "ragged", n=hk_adaptive.per_pixel(counts, W, H))
    assert (n == 2).any() and (stat >= 0).any()


# ---- 3: a threshold of 0 is the call as it was ------------------------------------------------------------------------------------------------------------
def test_threshold_zero_is_the_call_without_rejection():
    r = _scene("c1", 40, 36)
    assert r.denoise_reject == 0.0
    plain = ht.Replay()
    for i in range(3):
        _orbit(r, 1.0 * i)
        _frame(r, 5, seed=i + 1)
        r.denoise_temporal()
        hc, hv, hn = r.denoise_history()
        want = plain.frame(_camera(r), r.framebuffer(), r.variance(), r.features(), r.sample, r.denoise_alpha, r.denoise_iterations, tuple(r.denoise_sigma))
        assert _same(hc, want[0]) and _same(hv, want[1]) and _same(hn, want[2]) and _same(r.denoised(), want[3])
        with pytest.raises(volren_amd.VolrenError, match="denoise_reject_stat"):
            r.denoise_reject_stat()
    r.denoise_reject = 3.0                            # one call with it, then one without: the statistic is the last call's or nobody's
    _frame(r, 5, seed=9)
    r.denoise_temporal()
    assert r.denoise_reject_stat().shape == (36, 40)
    r.denoise()                                       # (the spatial filter has nothing to do with it)
    r.denoise_reject_stat()
    r.denoise_reject = 0.0
    r.denoise_temporal()
    with pytest.raises(volren_amd.VolrenError, match="denoise_reject_stat"):
        r.denoise_reject_stat()


# ---- 4: state rules -----------------------------------------------------------------------------------------------------------------------------------------
def test_what_keeps_and_what_drops_the_history_is_unchanged():
    """test_gpu_temporal's state test through the fetch / resolve kernels, with the threshold that never rejects, so that every length is known"""
    r = _scene("c1", 48, 40)
    r.denoise_reject = 2.0 ** 20
    with pytest.raises(volren_amd.VolrenError, match="denoise_reject_stat"):
        r.denoise_reject_stat()
    _frame(r, 4, seed=1, fseed=7)
    r.denoise_temporal()
    want = 1
    assert (r.denoise_history()[2] == want).all() and (r.denoise_reject_stat() == -1).all()
    for change in ("reset", "cam_pos", "envmap", "commit"):
        if change == "reset":
            r.reset()
        elif change == "cam_pos":
            r.cam_pos = r.cam_pos
        elif change == "envmap":
            r.load_envmap(scenes.HDR)
        else:
            r.commit()
        _frame(r, 4, seed=want + 1, fseed=7)
        r.denoise_temporal()
        want += 1
        assert (r.denoise_history()[2] == want).all(), change
        assert (r.denoise_reject_stat() >= 0).all(), change
    before = r.denoise_history()
    r.denoise()
    assert all(_same(a, b) for a, b in zip(before, r.denoise_history()))
    _orbit(r, 1.0)
    _frame(r, 4, seed=9, fseed=7)
    r.denoise_temporal()
    assert r.denoise_history()[2].max() == want + 1
    r.denoise_history_reset()                         # drops the history; the statistic of the last call stays readable
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    r.denoise_reject_stat()
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 1).all() and (r.denoise_reject_stat() == -1).all()
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 2).all()
    r.resize(40, 32)
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    with pytest.raises(volren_amd.VolrenError, match="denoise_reject_stat"):
        r.denoise_reject_stat()
    _frame(r, 4)
    r.denoise_temporal()
    assert r.denoise_history()[2].shape == (32, 40) and r.denoise_reject_stat().shape == (32, 40)


def test_the_threshold_is_range_checked():
    check_range(volren_amd.Renderer(16, 16))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_scratch_that_does_not_fit_fails_the_call_and_changes_nothing():
    lib = volren_amd.load()
    r = _scene("c1", 64, 48)
    for i in range(2):                                # both halves of the history pair and every buffer of the filter exist after these
        _frame(r, 4, seed=i + 1, fseed=7)
        r.denoise_temporal()
    before, result = r.denoise_history(), r.denoised()
    _frame(r, 4, seed=3, fseed=7)
    r.denoise_reject = 2.0 ** 20
    try:
        lib.vr_test_alloc_cap_mb(0)                   # the scratch between the two kernels is the one buffer still to allocate
        with pytest.raises(volren_amd.VolrenError, match="allocation cap"):
            r.denoise_temporal()
    finally:
        lib.vr_test_alloc_cap_mb(-1)
    assert all(_same(a, b) for a, b in zip(before, r.denoise_history()))
    assert _same(result, r.denoised())
    with pytest.raises(volren_amd.VolrenError, match="denoise_reject_stat"):
        r.denoise_reject_stat()
    r.denoise_temporal()                              # and with the memory back, the sequence goes on
    assert (r.denoise_history()[2] == 3).all() and (r.denoise_reject_stat() >= 0).all()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_three_logical_shards_equal_one_device():
    name, w, h, spp, fspp = "c2", 70, 52, 4, 3
    one = _scene(name, w, h)
    s = volren_amd.ShardedRenderer(w, h, [0, 0, 0])
    s.each(lambda p: scenes.configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    one.denoise_reject = 3.0
    s.parts[0].denoise_reject = 3.0                   # the filter's settings are part 0's
    assert s.denoise_reject == 3.0
    rejected = 0
    for frame in range(2):
        if frame == 1:
            def thinner(p):
                p.density_scale = 0.25 * p.density_scale
            thinner(one)
            s.each(thinner)
        for r in (one, s):
            r.reset()
            r.render(spp)
            r.render_features(fspp)
            r.denoise_temporal()
        assert _same(s.denoised(), one.denoised()), frame
        for a, b in zip(s.denoise_history(), one.denoise_history()):
            assert _same(a, b), frame
        assert _same(s.denoise_reject_stat(), one.denoise_reject_stat())
        rejected += int(ht.rejected(one.denoise_reject_stat(), 3.0).sum())
    assert rejected > 0
    one.close()
    s.close()


# ---- 7: what it is for ----------------------------------------------------------------------------------------------------------------------------------------
def test_rejection_follows_a_changing_scene_and_costs_nothing_on_a_steady_one():
    """tests/test_reject_host.py's scenario and bounds through volren_amd.Renderer: c2 at 64x48, 8 frames of 16 spp, seeds 100 .. 107, fixed camera,
    the scene changed before frame 4, against 1024 spp of seed 777 of the changed scene.  The pipeline is bit-exact, so the numbers are the CPU test's."""
    def scene(scenario):
        r = _scene("c2", W3, H3)
        change_scene(r, scenario)
        return r

    def render(r, i):
        _frame(r, SPP, seed=100 + i)

    def reference_of(scenario):
        r = scene(scenario)
        r.variance = 0
        r.seed = 777
        r.render(1024)
        return r.framebuffer()

    def spatial(scenario, i):
        r = scene(scenario)
        render(r, i)
        r.denoise()
        return r.denoised()

    def replay_of(tau):
        r = scene("steady")
        r.denoise_reject = tau
        state = {"changed": False}

        def one(cam, scenario, i):
            if i >= CHANGE and not state["changed"]:
                change_scene(r, scenario)
                state["changed"] = True
            render(r, i)
            r.denoise_temporal()
            return r.denoised(), (r.denoise_reject_stat() if tau > 0 else None)
        return one

    check_table(run_scenarios(lambda scenario, i: (scenario, i), reference_of, None, spatial, replay_of))


# ---- 8: Python, volpy, CLI --------------------------------------------------------------------------------------------------------------------------------------
def test_python_and_volpy_shapes_and_row_order():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.variance = 1
    assert vr.denoise_reject == 0.0
    vr.denoise_reject = 3.0
    assert vr.denoise_reject == 3.0 and vr._r.denoise_reject == 3.0
    replay = ht.Replay()
    r = vr._r
    for seed in (1, 2):                               # two frames of different samples: T is a picture, not a constant
        vr.seed = seed
        vr.render(6)
        vr.render_features(6)
        vr.denoise_temporal()
        want = replay.frame(_camera(r), r.framebuffer(), r.variance(), r.features(), r.sample, r.denoise_alpha, tau=3.0)
    t = r.denoise_reject_stat()
    assert t.shape == (24, 40) and t.dtype == np.float32
    assert _same(t, replay.stat) and not _same(t, replay.stat[::-1])      # row 0 = bottom, like every array the replay takes and gives
    raw = np.empty(24 * 40, np.float32)
    assert r._L.vr_denoise_reject_stat(r._h, raw.ctypes.data) == 0 and np.array_equal(raw, t.reshape(-1))
    td = vr.denoise_reject_stat_data()
    assert td.shape == (40, 24) == vr.fbo_data().shape[:2] and np.array_equal(td.reshape(-1), raw)
    assert _same(r.denoised(), want[3])


def test_cli_denoise_reject(tmp_path):
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "12", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    lib = volren_amd.load()
    folder = tmp_path / "anim"
    folder.mkdir()
    for i, s in enumerate((5, 6)):                    # a folder of two grid frames: the volume changes under a fixed camera
        f = scenes.synthetic_density(40, seed=s)
        assert lib.vr_write_brick_from_dense(f.ctypes.data, 40, 40, 40, None, str(folder / ("f%03d.brick" % i)).encode()) == 0

    def run(flags, png):
        return subprocess.run([exe, str(folder), scenes.HDR] + args + list(flags) + ["--output", png + ".png"], cwd=tmp_path, capture_output=True, text=True, timeout=300)

    for flags, png in ((("--denoise-temporal",), "t"), (("--denoise-temporal", "--denoise-reject", "0"), "t0"), (("--denoise-temporal", "--denoise-reject", "3"), "t3")):
        out = run(flags, png)
        assert out.returncode == 0, out.stderr[-2000:]
    for i in range(2):
        assert (tmp_path / ("t_%06d.png" % i)).read_bytes() == (tmp_path / ("t0_%06d.png" % i)).read_bytes()      # 0 = off
    assert (tmp_path / "t_000000.png").read_bytes() == (tmp_path / "t3_000000.png").read_bytes()                  # the first frame has no history to reject
    assert (tmp_path / "t_000001.png").read_bytes() != (tmp_path / "t3_000001.png").read_bytes()                  # the second rejects where the volume changed
    bad = run(("--denoise", "--denoise-reject", "3"), "bad")
    assert bad.returncode != 0 and "--denoise-reject needs --denoise-temporal" in bad.stderr
    bad = run(("--denoise-temporal", "--denoise-reject", "1e-9"), "bad")
    assert bad.returncode != 0 and "--denoise-reject" in bad.stderr and "2^-10" in bad.stderr
