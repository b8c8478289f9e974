"""CPU: the host build of the temporal accumulation's history rejection (volren_amd/csrc/vr_temporal.h steps 2a, 3a through
tests/hostkernel/temporal_host.cpp) against a float64 numpy statement of its rules (tests/hk_temporal.py spec_*) on synthetic histories and guides,
thresholds that never and always reject, thin frames behind range checks in the sanitizer build, and what it is for: a scene that changes under a
fixed camera, rendered by the oracle."""
import numpy as np
import pytest

import hk_denoise
import hk_features
import hk_temporal as ht
import scenes
from hk_common import bits as _bits
from test_temporal_host import orbit_camera, synthetic_guide, synthetic_history

SIZES = ((96, 72), (1, 1), (1, 37), (37, 1), (33, 31))
CAMERAS = (("moved", 10.0, 11.0), ("unchanged", 20.0, 20.0))      # degrees on test_temporal_host's orbit: the history's camera, the frame's


def _inputs(rng, W, H, a0, a1, smooth):
    """a frame and a history that mostly matches it (test_temporal_host's generators); NaN-free except for the history's 3 % NaN depths"""
    cur, prev = orbit_camera(a1, height=0.3), orbit_camera(a0, height=0.3 if a0 == a1 else 0.25)
    k, d = synthetic_guide(rng, W, H)
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    v = rng.uniform(0.0, 0.1, (H, W)).astype(np.float32)
    hc, rec = synthetic_history(rng, cur, prev, k, d, W, H, smooth=smooth)
    return cur, (prev, hc, rec), c, v, k, d


# ---- 1: the host build against the float64 statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", (3.0, 0.5))
@pytest.mark.parametrize("camera", CAMERAS, ids=lambda c: c[0])
@pytest.mark.parametrize("size", SIZES)
def test_statistic_and_decision_match_float64(size, camera, tau):
    """On a smooth history (neighbouring taps differ by under 1 %, so the coordinates' float32 error does not show in h), from the coordinates the host
    build found -- test_temporal_host holds those to the float64 reprojection -- so that both sides weigh the same taps.  The depth test of the
    generator's histories is never close (ratios 0, 0.03, 0.05, 0.23, 0.3 against 0.1), so `has` must agree everywhere.  T is a mean of up to 25
    non-negative terms (dl^2 / var), each with a relative error of a few 2^-24 x luma / |dl|; terms with small dl, where that is large, weigh little,
    and 1e-5 relative holds.  The decision is compared where T is not within 1e-4 of tau; C, V, N follow the host build's decision, as
    test_temporal_host's step test follows its coordinates."""
    W, H = size
    _, a0, a1 = camera
    left_out = pixels = 0
    kept = dropped = 0
    for seed in range(4):
        rng = np.random.default_rng(7000 + 31 * seed + W * 7 + H)
        cur, hist, c, v, k, d = _inputs(rng, W, H, a0, a1, smooth=True)
        same = a0 == a1
        alpha = (0.1, 2.0 ** -20, 1.0, 0.3)[seed]
        C, R, T = ht.step_reject(cur, c, v, k, d, alpha, tau, hist, checked=True)
        C2, R2, T2 = ht.step_reject(cur, c, v, k, d, alpha, tau, hist)
        assert np.array_equal(_bits(C), _bits(C2)) and np.array_equal(_bits(R), _bits(R2)) and np.array_equal(_bits(T), _bits(T2))
        given = None if same else ht.reproject(cur, hist[0], k, d)
        has, h, vh, nh = ht.spec_fetch(cur, k, d, hist, given=given)
        sT = ht.spec_stat(c, v, has, h, vh)
        assert np.array_equal(T != ht.NO_HISTORY, has)
        assert np.allclose(T[has], sT[has], rtol=1e-5, atol=0)
        near = has & (np.abs(sT - tau) <= 1e-4 * tau)
        rej = ht.rejected(T, tau)
        assert np.array_equal(rej[~near], (has & ~(sT <= tau))[~near])
        # C, V, N: the statement's blend where the host build kept the history, the frame where it did not
        sC, sV, sN = ht.spec_step(cur, c, v, k, d, alpha, hist, given=given)[:3]
        keep = has & ~rej
        assert np.array_equal(R[..., 1][keep], sN[keep].astype(np.float32)) and (R[..., 1][~keep] == 1).all()
        assert np.allclose(C[keep], sC[keep], rtol=1e-5, atol=1e-30) and np.allclose(R[..., 0][keep], sV[keep], rtol=1e-5, atol=1e-30)
        assert np.array_equal(_bits(C[~keep]), _bits(c[~keep])) and np.array_equal(_bits(R[..., 0][~keep]), _bits(v[~keep]))
        assert np.array_equal(_bits(R[..., 2]), _bits(k)) and np.array_equal(_bits(R[..., 3]), _bits(d))
        left_out += int(near.sum())
        pixels += W * H
        kept += int(keep.sum())
        dropped += int(rej.sum())
    print("%dx%d %s tau %g: %d of %d pixels left out, %d kept, %d rejected" % (W, H, camera[0], tau, left_out, pixels, kept, dropped))
    assert left_out <= 0.01 * pixels
    if W * H >= 1000 and tau == 3.0:
        assert kept > 0.05 * pixels and dropped > 0.05 * pixels      # both outcomes are exercised


def test_the_window_counts_only_pixels_with_a_history_inside_the_frame():
    """by hand, unchanged camera: z2 = 4 at every pixel with a history except one of 104; the pixels of a column have none"""
    W, H = 9, 7
    cam = orbit_camera(0.0)
    k = np.full((H, W), 0.5, np.float32)
    d = np.ones((H, W), np.float32)
    w = np.asarray(ht.LUMA)
    c = np.zeros((H, W, 4), np.float32)
    hc = np.zeros((H, W, 4), np.float32)
    hc[..., 1] = 2.0
    hc[3, 4, 1] = 10.0
    v = np.full((H, W), 0.25, np.float32)
    rec = np.stack([np.full((H, W), 0.25, np.float32), np.full((H, W), 3.0, np.float32), k, d], axis=-1)
    rec[:, 6, 1] = 0.0                                   # column 6: no history
    C, R, T = ht.step_reject(cam, c, v, k, d, 0.1, 5.0, (cam, hc, rec), checked=True)
    z = ((hc[..., :3].astype(np.float64) * w).sum(-1)) ** 2 / 0.5
    assert (T[:, 6] == -1).all() and (R[:, 6, 1] == 1).all()
    for (x, y) in ((0, 0), (8, 6), (4, 3), (2, 3), (1, 3), (7, 0)):
        ys, xs = range(max(y - 2, 0), min(y + 3, H)), [q for q in range(max(x - 2, 0), min(x + 3, W)) if q != 6]
        want = sum(z[j, i] for j in ys for i in xs) / (len(ys) * len(xs))
        assert abs(T[y, x] - want) <= 3e-6 * want, (x, y, T[y, x], want)      # 25 additions of 2^-24 each
    assert T[3, 4] > 5.0 and R[3, 4, 1] == 1 and np.array_equal(C[3, 4], c[3, 4])      # rejected: the frame
    assert T[3, 1] < 5.0 and R[3, 1, 1] == 4                                            # outside the window of (4, 3): kept


# ---- 2: thresholds that never and always reject ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", CAMERAS, ids=lambda c: c[0])
@pytest.mark.parametrize("size", SIZES)
def test_the_largest_threshold_is_the_step_without_rejection_and_the_smallest_rejects_all(size, camera):
    W, H = size
    rng = np.random.default_rng(8000 + W * 7 + H)
    cur, hist, c, v, k, d = _inputs(rng, W, H, camera[1], camera[2], smooth=False)
    C0, R0 = ht.step(cur, c, v, k, d, 0.1, hist)
    C, R, T = ht.step_reject(cur, c, v, k, d, 0.1, ht.TAU_MAX, hist, checked=True)
    assert not np.isnan(T).any() and T.max() <= ht.TAU_MAX
    assert np.array_equal(_bits(C), _bits(C0)) and np.array_equal(_bits(R), _bits(R0))
    has = T != ht.NO_HISTORY
    assert np.array_equal(has, R0[..., 1] > 1)
    C, R, T = ht.step_reject(cur, c, v, k, d, 0.1, ht.TAU_MIN, hist, checked=True)
    assert np.array_equal(T != ht.NO_HISTORY, has) and (T[has] > ht.TAU_MIN).all()      # a white-noise history differs from the frame everywhere
    assert np.array_equal(_bits(C), _bits(c))
    assert np.array_equal(_bits(R), _bits(np.stack([v, np.ones_like(v), k, d], axis=-1)))
    assert ht.reject_constants() == (2.0 ** -10, 2.0 ** 20, float(np.float32(1e-12)), 2.0, -1.0)


def test_a_nan_rejects_and_the_first_frame_is_the_frame():
    W, H = 33, 31
    rng = np.random.default_rng(9)
    cam = orbit_camera(5.0)
    k, d = synthetic_guide(rng, W, H)
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    v = rng.uniform(0.0, 0.1, (H, W)).astype(np.float32)
    C, R, T = ht.step_reject(cam, c, v, k, d, 0.1, 3.0, None, checked=True)
    assert (T == -1).all() and np.array_equal(_bits(C), _bits(c)) and np.array_equal(_bits(R), _bits(np.stack([v, np.ones_like(v), k, d], axis=-1)))
    rec = np.stack([v, np.full((H, W), 2.0, np.float32), k, d], axis=-1)
    hc = c.copy()                                        # the history is the frame: z2 = 0, nothing rejected ...
    hc[10, 12, 1] = np.nan                               # ... but for the 5 x 5 pixels whose window holds the NaN
    C, R, T = ht.step_reject(cam, c, v, k, d, 0.1, ht.TAU_MAX, (cam, hc, rec), checked=True)
    hole = np.zeros((H, W), bool)
    hole[8:13, 10:15] = True
    assert np.isnan(T[hole]).all() and (T[~hole] == 0).all()
    assert (R[..., 1][hole] == 1).all() and (R[..., 1][~hole] == 3).all()
    assert np.array_equal(_bits(C[hole]), _bits(c[hole]))


# ---- 4: the thin sizes behind range checks, in the sanitizer build ------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ((1, 1), (1, 37), (37, 1), (2, 3), (33, 31)))
def test_no_window_or_history_read_leaves_the_frame(size):
    W, H = size
    rng = np.random.default_rng(9000 + W * 7 + H)
    for yaw, fov, a0, a1 in ((0.0, 40.0, 10.0, 12.0), (25.0, 40.0, 10.0, 12.0), (180.0, 40.0, 10.0, 12.0), (0.0, 70.0, 3.0, 3.0), (-40.0, 20.0, 10.0, 10.5)):
        cur, prev = orbit_camera(a1, fov=fov, yaw_deg=yaw), orbit_camera(a0)
        k, d = synthetic_guide(rng, W, H)
        if W * H > 4:
            d[rng.random((H, W)) < 0.05] = np.nan
        c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
        v = rng.uniform(0.0, 0.1, (H, W)).astype(np.float32)
        hc, rec = synthetic_history(rng, cur, prev, k, np.nan_to_num(d, nan=1.0), W, H, smooth=False)
        for tau in (3.0, 0.5):
            C, R, T = ht.step_reject(cur, c, v, k, d, 0.1, tau, (prev, hc, rec), checked=True)      # asserts that no read fell outside
            C2, R2, T2 = ht.step_reject(cur, c, v, k, d, 0.1, tau, (prev, hc, rec))
            assert np.array_equal(_bits(C), _bits(C2)) and np.array_equal(_bits(R), _bits(R2)) and np.array_equal(_bits(T), _bits(T2))


# ---- 3: what it is for ------------------------------------------------------------------------------------------------------------------------------
W3, H3, SPP, FRAMES, CHANGE = 64, 48, 16, 8, 4
SCENARIOS = ("steady", "env_strength", "density_scale")


def change_scene(r, scenario):
    """what happens before frame CHANGE (r: an oracle or a HIP renderer of c2)"""
    if scenario == "env_strength":
        r.env_strength = 3.0 * r.env_strength
    elif scenario == "density_scale":
        r.density_scale = 0.25 * r.density_scale


def run_scenarios(frame_of, reference_of, camera, denoise_spatial, replay_of):
    """The table of DESIGN.md 5 for one renderer.  frame_of(scenario, i) -> (colour, variance, features) of frame i (seed 100 + i; the scene changed as
    `scenario` says from frame CHANGE on), reference_of(scenario) -> the changed scene at 1024 spp of seed 777.  -> per scenario and tau (0, 3):
    errors of frames CHANGE .. (relative L2 of RGB), outputs, rejected shares of every frame; and the spatial filter's errors and outputs."""
    out = {}
    for s in SCENARIOS:
        ref = reference_of(s)[..., :3]
        frames = [frame_of("steady" if i < CHANGE else s, i) for i in range(FRAMES)]
        res = {"spatial": [], "spatial_out": []}
        for i in range(CHANGE, FRAMES):
            sp = denoise_spatial(*frames[i])
            res["spatial"].append(scenes.rel_l2(sp[..., :3], ref))
            res["spatial_out"].append(sp)
        for tau in (0.0, 3.0):
            rp = replay_of(tau)
            err, outs, share = [], [], []
            for i in range(FRAMES):
                o, stat = rp(camera, *frames[i])
                if i >= CHANGE:
                    err.append(scenes.rel_l2(o[..., :3], ref))
                    outs.append(o)
                share.append(float(ht.rejected(stat, tau).mean()) if tau > 0 and stat is not None else 0.0)
            res[tau] = dict(err=err, out=outs, share=share)
        out[s] = res
        print("%-14s spatial %s | tau 0 %s | tau 3 %s | rejected %s" % (s, " ".join("%.4f" % e for e in res["spatial"]), " ".join("%.4f" % e for e in res[0.0]["err"]),
                                                                        " ".join("%.4f" % e for e in res[3.0]["err"]), " ".join("%.1f%%" % (100 * x) for x in res[3.0]["share"])))
    return out


def check_table(t):
    """The bounds: halfway between what was measured on the CPU (the float32 host build around oracle frames; see the test's docstring) and neutral."""
    steady, env, den = t["steady"], t["env_strength"], t["density_scale"]
    assert steady[3.0]["err"][-1] <= 1.05 * steady[0.0]["err"][-1]
    assert np.array_equal(_bits(env[3.0]["out"][0]), _bits(env["spatial_out"][0]))       # every pixel rejected: frame CHANGE is the spatial filter's
    assert env[3.0]["err"][-1] <= 0.86 * env["spatial"][-1]
    assert env[0.0]["err"][-1] > 3.0 * env["spatial"][-1]                                # the scenario bites
    assert den[3.0]["err"][-1] <= 0.94 * den[0.0]["err"][-1]
    assert max(steady[3.0]["share"]) <= 0.02
    assert max(env[3.0]["share"][:CHANGE] + env[3.0]["share"][CHANGE + 1:]) <= 0.02 and max(den[3.0]["share"][:CHANGE] + den[3.0]["share"][CHANGE + 1:]) <= 0.02      # every frame without a change before it


@pytest.fixture(scope="module")
def table():
    from test_gpu_features import _oracle_radiance, _replay
    cache = {}

    def scene(scenario):
        o = scenes.oracle_scene("c2", W3, H3)
        change_scene(o, scenario)
        return o

    def frame_of(scenario, i):
        if (scenario, i) not in cache:
            o = scene(scenario)
            o.seed = 100 + i
            mu, S = _replay(_oracle_radiance(o, SPP))
            var = (S * (np.float32(SPP) / np.float32(SPP - 1))).astype(np.float32)
            cache[(scenario, i)] = (mu, var, hk_features.feature_pass(o, SPP))
        return cache[(scenario, i)]

    def reference_of(scenario):
        o = scene(scenario)
        o.seed = 777
        return o.render(1024).copy()

    def replay_of(tau):
        rp = ht.Replay()

        def one(cam, color, var, feat):
            out = rp.frame(cam, color, var, feat, SPP, 0.1, tau=tau)[3]
            return out, rp.stat
        return one

    o = scene("steady")
    p = o.params()
    cam = ht.camera(list(p.cam_pos), list(p.cam_transform), fov_degree=o.cam_fov)
    return run_scenarios(frame_of, reference_of, cam, lambda c, var, f: hk_denoise.denoise(c, var, f, SPP), replay_of)


def test_rejection_follows_a_changing_scene_and_costs_nothing_on_a_steady_one(table):
    """c2 at 64x48, 8 frames of 16 spp (features 16 spp), seeds 100 .. 107, fixed camera, alpha 0.1, default sigmas, 5 iterations; the scene changes
    before frame 4; relative L2 of RGB against 1024 spp of seed 777 of the changed scene.  Measured (frames 4 .. 7: spatial only | tau 0 | tau 3 | pixels with a history rejected in frames 0 .. 7):
      steady         0.0584 0.0553 0.0551 0.0556 | 0.0406 0.0398 0.0385 0.0374 | 0.0406 0.0398 0.0393 0.0377 | at most 0.2 % each
      env_strength   0.0568 0.0543 0.0554 0.0557 | 0.5210 0.4307 0.3688 0.3217 | 0.0568 0.0478 0.0431 0.0405 | 98.0 % at frame 4 (the rest has no history), 0 otherwise
      density_scale  0.0554 0.0516 0.0550 0.0562 | 0.0621 0.0553 0.0494 0.0457 | 0.0527 0.0454 0.0414 0.0399 | 5.6 % at frame 4, at most 0.2 % after
    so the ratios the bounds are about are 1.008 (steady, tau 3 over tau 0), 0.727 and 5.8 (env_strength, tau 3 and tau 0 over spatial) and 0.873
    (density_scale, tau 3 over tau 0)."""
    check_table(table)
