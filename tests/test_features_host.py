"""CPU: the denoiser feature pass of the lane code (vr_trace.h feature_sample / feature_pixel), host-compiled, against the oracle's
orc_sample_volume (the first segment of sample_volumeDDA, common.glsl:458-501) on the draws of colour sample s: hit, distance and albedo
bit for bit; normals against a float64 central difference of the decoded grid; the per-pixel pass against float32 sums in sample order."""
import ctypes as C

import numpy as np
import pytest

import hk_features
import scenes
from oracle import binding as ob

W, H, SPP = 64, 48, 4
SCENES = ("c1", "c3", "c4_64", "c5_64")          # smoke.brick, + lut.txt, dense fp16 grid, brick grids with an emission grid


def _oracle_samples(o, spp):
    L = ob.lib()
    L.orc_sample_volume.argtypes = [C.POINTER(ob.Params), C.POINTER(ob.Scene), ob.P_f, ob.P_f, ob.P_u32, ob.P_f]
    L.orc_sample_volume.restype = C.c_int
    L.orc_view_dir.argtypes = [C.POINTER(ob.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, ob.P_f]
    p, s = o.params(), o.scene()
    pos = np.array(o.cam_pos, np.float32)
    hit = np.zeros((o.h, o.w, spp), bool)
    val = np.zeros((o.h, o.w, spp, 4), np.float32)
    dirs = np.zeros((o.h, o.w, spp, 3), np.float32)
    seed = C.c_uint32()
    d = np.zeros(3, np.float32)
    out = np.zeros(4, np.float32)
    for y in range(o.h):
        for x in range(o.w):
            for k in range(spp):
                seed.value = L.orc_tea((p.seed * (y * o.w + x)) & 0xFFFFFFFF, k + 1, 32)
                jx = L.orc_rng(C.byref(seed))
                jy = L.orc_rng(C.byref(seed))
                L.orc_view_dir(C.byref(p), x, y, o.w, o.h, jx, jy, ob.fptr(d))
                out[:] = 0
                hit[y, x, k] = L.orc_sample_volume(C.byref(p), C.byref(s), ob.fptr(pos), ob.fptr(d), C.byref(seed), ob.fptr(out)) != 0
                val[y, x, k] = out
                dirs[y, x, k] = d
    return hit, val, dirs, p


def _fma(a, b, c):
    """float32 fma (the float64 product of two floats is exact)."""
    return (np.float64(1.0) * np.asarray(a, np.float32) * np.asarray(b, np.float32) + np.asarray(c, np.float32)).astype(np.float32)


@pytest.fixture(scope="module", params=SCENES)
def scene(request):
    o = scenes.oracle_scene(request.param, W, H)
    return request.param, o


def test_feature_samples_match_the_oracle_bitwise(scene):
    name, o = scene
    hit, val = hk_features.samples(o, SPP)
    ohit, oval, _, _ = _oracle_samples(o, SPP)
    assert np.array_equal(hit, ohit), (name, int((hit != ohit).sum()))
    assert 0 < hit.mean() < 1, "want both pixels that hit and samples that miss"
    assert (~hit.any(axis=2)).any(), "some pixels must miss the volume altogether"
    # t and albedo (= the oracle's throughput after the real collision) bit for bit
    assert np.array_equal(val[hit][:, 0:4].view(np.uint32), oval[hit].view(np.uint32)), name


def test_feature_normals_match_a_float64_central_difference(scene):
    name, o = scene
    hit, val = hk_features.samples(o, SPP)
    _, _, dirs, p = _oracle_samples(o, SPP)
    minv = np.array(p.vol_density_inv_transform, np.float64)
    # the collision point as the tracker forms it, in float32 (vr_math.h mat4_point / mat4_dir, axpy): only the filter is evaluated in float64
    m = np.array(p.vol_density_inv_transform, np.float32)
    pos = np.array(o.cam_pos, np.float32)
    ipos = np.array([_fma(m[8 + r], pos[2], _fma(m[4 + r], pos[1], _fma(m[r], pos[0], m[12 + r]))) for r in range(3)], np.float32)
    d = dirs[hit]
    idir = np.stack([_fma(m[8 + r], d[:, 2], _fma(m[4 + r], d[:, 1], (m[r] * d[:, 0]).astype(np.float32))) for r in range(3)], 1)
    ip = _fma(val[hit][:, 0:1], idir, ipos[None, :]).astype(np.float64)
    grid = hk_features.decoded_grid(o.density)
    ref, gl = hk_features.normals_f64(grid, minv, ip)
    got = val[hit][:, 4:7]
    well = gl > 1e-2 * grid.max()
    assert well.sum() > 100, (name, int(well.sum()))
    err = np.abs(got[well] - ref[well]).max()
    assert err <= 1e-4, (name, err)
    assert np.allclose(np.linalg.norm(got[well], axis=1), 1.0, atol=1e-5)
    assert np.all(np.isfinite(got))


def test_feature_pass_is_the_float32_sum_in_sample_order(scene):
    name, o = scene
    hit, val = hk_features.samples(o, SPP)
    fp = hk_features.feature_pass(o, SPP)
    ref = hk_features.aggregate(hit, val)
    assert np.array_equal(fp.view(np.uint32), ref.view(np.uint32)), name
    assert np.array_equal(fp[..., 3], (hit.sum(axis=2) / np.float32(SPP)).astype(np.float32))
    assert np.all(fp[~hit.any(axis=2)] == 0)


_FAR = r"""
import sys
sys.path[:0] = [%(tests)r, %(root)r]
import numpy as np
import hk_features, scenes
o = scenes.oracle_scene("c1", 8, 8)
o.cam_pos = tuple(float(v) * %(k)r for v in o.cam_pos)
o.cam_fov = 70.0 / %(k)r
hit, _ = hk_features.samples(o, 2, raw=True)
fp, lost = hk_features.feature_pass(o, 2, with_lost=True)
print(" ".join(str(int(v)) for v in np.bincount(hit.ravel(), minlength=3)), int((hit == 2).any(axis=2).sum()), lost, int(np.isfinite(fp).all()))
"""


@pytest.mark.parametrize("k", (1e5, 1e6, 1e7))
def test_far_camera_returns(k):
    """A camera so far away that t + dt rounds back to t: the reference's tracker never ends there (empty cells: nothing changes; a cell whose
    collision point has no density: null collisions for ever).  The lane code must return: a step that changes nothing ends the segment without
    a collision, anything else is given up after kFeatureMaxSteps and reported (the pixel stops there)."""
    import os
    import subprocess
    import sys
    code = _FAR % dict(tests=os.path.dirname(os.path.abspath(__file__)), root=scenes.ROOT, k=k)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stderr[-2000:]
    miss, hit, lost, lost_px, pass_lost, finite = (int(v) for v in out.stdout.split()[-6:])
    assert miss + hit + lost == 8 * 8 * 2 and finite == 1
    assert lost_px == pass_lost                     # the pass reports exactly the pixels with a lost sample
    if k >= 1e7:
        assert lost == 0 and hit == 0               # every segment stalls in an empty cell: fixed points, ended as misses


def test_near_far_camera_still_matches_the_oracle():
    """The bound changes nothing where the reference's tracker ends: a camera 1000x further out (and 1000x narrower) is still bit-exact."""
    o = scenes.oracle_scene("c1", 16, 12)
    o.cam_pos = tuple(float(v) * 1e3 for v in o.cam_pos)
    o.cam_fov = 70.0 / 1e3
    hit, val = hk_features.samples(o, 2, raw=True)
    ohit, oval, _, _ = _oracle_samples(o, 2)
    assert not (hit == 2).any() and np.array_equal(hit == 1, ohit)
    h = hit == 1
    assert h.any() and np.array_equal(val[h][:, 0:4].view(np.uint32), oval[h].view(np.uint32))
