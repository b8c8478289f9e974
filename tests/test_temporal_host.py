"""CPU: the host build of the temporal accumulation (volren_amd/csrc/vr_temporal.h through tests/hostkernel/temporal_host.cpp) against a float64 numpy
statement of its rules (tests/hk_temporal.py spec_*), on synthetic histories and guides: the reprojection, the tap rules, the blend, the unchanged
camera, the first frame, frames one pixel thin, cameras that look away."""
import numpy as np
import pytest

from hk_common import bits as _bits
import hk_temporal as ht

SIZES = ((96, 72), (1, 1), (1, 37), (37, 1), (33, 31), (256, 256))
# Largest |u32 - u64| / |w32 - w64| in pixels that test_reprojection_matches_float64 measures for its own seeded inputs, per frame size: a property of
# float32 at |u| <= W (the error grows with the coordinate), not of any device.  The tolerance is 4 x the measured value.
MEASURED_PX = {(96, 72): 1.69e-5, (1, 1): 5.26e-8, (1, 37): 3.51e-6, (37, 1): 7.87e-6, (33, 31): 5.65e-6, (256, 256): 5.54e-5}
TOL_PX = {k: 4.0 * v for k, v in MEASURED_PX.items()}


def orbit_camera(angle_deg, fov=40.0, radius=np.sqrt(2.0), height=0.0, yaw_deg=0.0):
    """A camera on a circle about +y through the origin, looking at the origin (yaw_deg: turned away from it about +y); 13 float32."""
    a = np.radians(angle_deg)
    pos = np.array([radius * np.sin(a), height, radius * np.cos(a)])
    fwd = -pos / np.linalg.norm(pos)
    y = np.radians(yaw_deg)
    fwd = np.array([np.cos(y) * fwd[0] + np.sin(y) * fwd[2], fwd[1], -np.sin(y) * fwd[0] + np.cos(y) * fwd[2]])
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return ht.camera(pos, np.concatenate([right, up, -fwd]), fov)      # columns: right, up, -forward (the camera looks down -z)


def synthetic_guide(rng, W, H):
    """coverage (a third of the pixels environment only) and depth in [0.8, 2], a few of them NaN"""
    k = np.where(rng.random((H, W)) < 0.33, 0.0, rng.uniform(0.1, 1.0, (H, W))).astype(np.float32)
    d = np.where(k > 0, rng.uniform(0.8, 2.0, (H, W)), 0.0).astype(np.float32)
    return k, d


PAIRS = ((0.0, 0.5), (10.0, 11.0), (45.0, 43.0), (200.0, 205.0), (-30.0, -27.0))      # degrees on the orbit: 0.5 .. 5 apart


@pytest.mark.parametrize("size", SIZES)
def test_reprojection_matches_float64(size):
    W, H = size
    rng = np.random.default_rng(1000 + W * 7 + H)
    worst = 0.0
    for a0, a1 in PAIRS:
        cur, prev = orbit_camera(a1, height=0.3), orbit_camera(a0, height=0.25)
        k, d = synthetic_guide(rng, W, H)
        u, w, dp, ok = ht.reproject(cur, prev, k, d)
        su, sw, sdp, front = ht.spec_reproject(cur, prev, k, d)
        assert np.array_equal(ok, front)
        ok &= (su >= -1) & (su <= W) & (sw >= -1) & (sw <= H)      # where a tap can lie inside the frame (a 37 x 1 frame is so wide that its outermost
        assert ok.any()                                             # rays land thousands of pixels away, or miss the other camera's half space)
        worst = max(worst, float(np.abs(u - su)[ok].max()), float(np.abs(w - sw)[ok].max()))
        hit = (k > 0) & ok
        assert np.allclose(dp[hit], sdp[hit], rtol=1e-6, atol=0)
    print("reprojection %dx%d: largest difference %.3g px (tolerance %.3g)" % (W, H, worst, TOL_PX[size]))
    assert worst <= TOL_PX[size], (size, worst)


def synthetic_history(rng, cur, prev, k, d, W, H, smooth):
    """A history that mostly matches what `cur` sees: depths of the reprojected points with a few percent of noise (some taps fail the 0.1 bound, most
    pass), the same kind of pixel mostly, lengths 0 .. 7, some NaN depths.  smooth: colour and variance are a slowly varying field (at most 0.5 % from
    one pixel to the next) instead of white noise -- see _compare_step."""
    hc = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    V = rng.uniform(0.0, 0.1, (H, W))
    if smooth:
        y, x = np.mgrid[0:H, 0:W]
        base = 1.0 + 0.5 * np.sin(0.01 * x + rng.uniform(0, 6)) * np.cos(0.01 * y + rng.uniform(0, 6))
        hc = (base[..., None] * np.array([1.0, 0.8, 0.6, 1.0])).astype(np.float32)
        V = 0.05 * base
    _, _, sdp, _ = ht.spec_reproject(cur, prev, k, d)
    K = np.where(rng.random((H, W)) < 0.1, np.where(k > 0, 0.0, 0.5), k)
    D = np.where(K > 0, np.where(k > 0, sdp, 1.4) * rng.choice([1.0, 1.0, 1.0, 1.03, 0.95, 1.3, 0.7], (H, W)), 0.0)
    D = np.where((rng.random((H, W)) < 0.03) & (K > 0), np.nan, D)
    N = rng.integers(0, 8, (H, W)).astype(np.float64)
    rec = np.stack([V, N, K, D], axis=-1).astype(np.float32)
    return hc, rec


def _compare_step(cur, prev, W, H, rng, alpha, tol_px, nan_depth=True, end_to_end=True):
    """One accumulation step of the host build against the float64 statement; -> (pixels left out, pixels, the statement's N).
    end_to_end: steps 1-4, the statement reprojecting in float64.  The two then blend the same taps with weights that differ by the coordinates' own
    error du (up to tol_px / 4), which moves h by du x (the difference between neighbouring taps) / (sum b): held to 1e-5 relative, that needs a history
    whose neighbours differ by well under 1 %, so this mode runs on a smooth field.  White-noise histories are compared with end_to_end = False: steps 2-4
    alone, the statement taking (u, w, d') from the host build's step 1, which test_reprojection_matches_float64 holds to tol_px."""
    k, d = synthetic_guide(rng, W, H)
    if nan_depth and W * H > 4:
        d[rng.random((H, W)) < 0.02] = np.nan
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    v = rng.uniform(0.0, 0.1, (H, W)).astype(np.float32)
    hc, rec = synthetic_history(rng, cur, prev, k, np.nan_to_num(d, nan=1.0), W, H, smooth=end_to_end)
    hist = (prev, hc, rec)
    C, R = ht.step(cur, c, v, k, d, alpha, hist, checked=True)
    C2, R2 = ht.step(cur, c, v, k, d, alpha, hist)
    assert np.array_equal(_bits(C), _bits(C2)) and np.array_equal(_bits(R), _bits(R2))      # the range-checked build computes the same
    sC, sV, sN, su, sw, ratio, sum_b = ht.spec_step(cur, c, v, k, d, alpha, hist, given=None if end_to_end else ht.reproject(cur, prev, k, d))
    assert np.array_equal(_bits(R[..., 2]), _bits(k)) and np.array_equal(_bits(R[..., 3]), _bits(d))
    with np.errstate(invalid="ignore"):
        near_tap = (np.abs(su - np.round(su)) <= tol_px) | (np.abs(sw - np.round(sw)) <= tol_px) if end_to_end else np.zeros((H, W), bool)
        near_bound = (np.abs(ratio - ht.DEPTH_BOUND) <= 1e-5).any(axis=-1)
    # (a third decision of the same kind: the taps that count weigh 2^-10 together, give or take the coordinates' error)
    near_weight = np.abs(sum_b - ht.MIN_WEIGHT) <= 2.0 * tol_px if end_to_end else np.zeros((H, W), bool)
    out = near_tap | near_bound | near_weight
    keep = ~out
    assert np.array_equal(R[..., 1][keep], sN[keep].astype(np.float32))
    assert np.allclose(C[keep], sC[keep], rtol=1e-5, atol=1e-30)
    assert np.allclose(R[..., 0][keep], sV[keep], rtol=1e-5, atol=1e-30)
    return int(out.sum()), W * H, sN


@pytest.mark.parametrize("end_to_end", (True, False))
@pytest.mark.parametrize("size", SIZES)
def test_step_matches_float64(size, end_to_end):
    W, H = size
    rng = np.random.default_rng(2000 + W * 7 + H)
    left_out = pixels = 0
    lengths = []
    for a0, a1 in PAIRS:
        for alpha in (0.1, 2.0 ** -20, 1.0) if W * H < 10000 else (0.1,):      # (the float64 statement is a Python loop over the pixels)
            o, n, sN = _compare_step(orbit_camera(a1, height=0.3), orbit_camera(a0, height=0.25), W, H, rng, alpha, TOL_PX[size], end_to_end=end_to_end)
            left_out += o
            pixels += n
            lengths.append(sN)
    print("step %dx%d: %d of %d pixels left out" % (W, H, left_out, pixels))
    assert left_out <= 0.01 * pixels or pixels < 100 and left_out == 0
    if W * H >= 1000:
        sN = np.concatenate([x.reshape(-1) for x in lengths])
        assert (sN == 1).mean() > 0.05 and (sN > 1).mean() > 0.3      # both outcomes are exercised


@pytest.mark.parametrize("size", ((1, 37), (37, 1), (33, 31), (96, 72)))
def test_taps_off_the_frame_and_cameras_that_look_away(size):
    W, H = size
    rng = np.random.default_rng(3000 + W * 7 + H)
    seen = set()
    for yaw, fov in ((25.0, 40.0), (-40.0, 40.0), (100.0, 40.0), (180.0, 40.0), (0.0, 70.0), (3.0, 20.0)):
        cur, prev = orbit_camera(12.0, fov=fov, yaw_deg=yaw), orbit_camera(10.0)
        k, d = synthetic_guide(rng, W, H)
        u, w, _, ok = ht.reproject(cur, prev, k, d)
        _, _, _, front = ht.spec_reproject(cur, prev, k, d)
        assert np.array_equal(ok, front)
        if not ok.all():
            seen.add("behind")
        if ok.any() and ((u[ok] < -1) | (u[ok] >= W) | (w[ok] < -1) | (w[ok] >= H)).any():
            seen.add("off")
        _, _, sN = _compare_step(cur, prev, W, H, rng, 0.1, TOL_PX[size], end_to_end=False)
        if yaw == 180.0:
            assert (sN == 1).all()                        # q.z >= 0 everywhere: nobody has a history
    assert seen == {"behind", "off"}


def test_unchanged_camera_reads_its_own_pixel_bit_for_bit():
    W, H = 33, 31
    rng = np.random.default_rng(5)
    cam = orbit_camera(20.0)
    k, d = synthetic_guide(rng, W, H)
    c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    v = rng.uniform(0.0, 0.1, (H, W)).astype(np.float32)
    hc = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
    N = rng.integers(0, 5, (H, W)).astype(np.float32)
    rec = np.stack([rng.uniform(0.0, 0.1, (H, W)).astype(np.float32), N, k, d], axis=-1)      # the same guide: every tap with N >= 1 counts
    rec[3, 4, 2] = 0.0 if k[3, 4] > 0 else 0.5                    # another kind of thing: no history there
    alpha = np.float32(0.1)
    C, R = ht.step(cam, c, v, k, d, alpha, (cam.copy(), hc, rec), checked=True)
    counts = N >= 1
    counts[3, 4] = False
    Nn = np.minimum(N + np.float32(1), np.float32(2.0 ** 20))
    a = np.maximum(alpha, np.float32(1) / Nn).astype(np.float32)
    oma = (np.float32(1) - a).astype(np.float32)
    want = (oma[..., None] * hc).astype(np.float32) + (a[..., None] * c).astype(np.float32)
    wantV = ((oma * oma).astype(np.float32) * rec[..., 0]).astype(np.float32) + ((a * a).astype(np.float32) * v).astype(np.float32)
    assert counts.any() and (~counts).any()
    assert np.array_equal(_bits(C[counts]), _bits(want[counts]))
    assert np.array_equal(_bits(R[..., 0][counts]), _bits(wantV[counts]))
    assert np.array_equal(R[..., 1][counts], Nn[counts])
    assert np.array_equal(_bits(C[~counts]), _bits(c[~counts])) and np.array_equal(_bits(R[..., 0][~counts]), _bits(v[~counts]))
    assert (R[..., 1][~counts] == 1).all()
    # a camera that differs in its last bit is reprojected instead (and lands within a hair of the pixel centres)
    moved = cam.copy()
    moved[0] = np.nextafter(moved[0], np.float32(10))
    u, w, _, ok = ht.reproject(moved, cam, k, d)
    assert ok.all() and np.abs(u - np.arange(W)[None, :]).max() < 1e-3 and np.abs(w - np.arange(H)[:, None]).max() < 1e-3


def test_first_frame_is_the_frame():
    for W, H in SIZES[:5]:
        rng = np.random.default_rng(6)
        k, d = synthetic_guide(rng, W, H)
        c = rng.uniform(0.0, 2.0, (H, W, 4)).astype(np.float32)
        v = rng.uniform(0.0, 0.1, (H, W)).astype(np.float32)
        C, R = ht.step(orbit_camera(0.0), c, v, k, d, 0.1, None, checked=True)
        assert np.array_equal(_bits(C), _bits(c))
        assert np.array_equal(_bits(R), _bits(np.stack([v, np.ones_like(v), k, d], axis=-1)))


def test_history_length_is_capped_and_alpha_floors_the_weight():
    W, H = 4, 3
    cam = orbit_camera(0.0)
    k = np.full((H, W), 0.5, np.float32)
    d = np.full((H, W), 1.0, np.float32)
    c = np.full((H, W, 4), 2.0, np.float32)
    hc = np.zeros((H, W, 4), np.float32)
    v = np.zeros((H, W), np.float32)
    rec = np.stack([v, np.full((H, W), 2.0 ** 20, np.float32), k, d], axis=-1)
    C, R = ht.step(cam, c, v, k, d, 2.0 ** -20, (cam, hc, rec))
    assert (R[..., 1] == 2.0 ** 20).all() and (C == np.float32(2.0 ** -19)).all()
    C, R = ht.step(cam, c, v, k, d, 0.25, (cam, hc, rec))
    assert (C == 0.5).all()
    assert ht.constants() == (np.float32(0.1), 2.0 ** -20, 1.0, np.float32(0.1), 2.0 ** -10, 2.0 ** 20)
