"""GPU: the a-trous denoiser (vr_denoise / vr_denoised) bit for bit against the host-compiled lane code (tests/hostkernel/denoise_host.cpp, itself held
to a float64 statement of the filter by tests/test_denoise_host.py), fed with the renderer's own framebuffer, variance and features; what it leaves
alone; its refusals; its noise reduction; the Python, volpy and CLI interfaces."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from hk_common import bits as _bits
import hk_denoise
import scenes
import volren_amd

pytestmark = pytest.mark.gpu


def _ready(name, w, h, spp, fspp=None):
    r = scenes.hip_scene(name, w, h)
    r.variance = 1
    r.render(spp)
    r.render_features(fspp or spp)
    return r


def _host(r, iterations=None, sigma=None):
    it = r.denoise_iterations if iterations is None else iterations
    sg = tuple(r.denoise_sigma) if sigma is None else sigma
    return hk_denoise.denoise(r.framebuffer(), r.variance(), r.features(), r.sample, it, sg)


@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
@pytest.mark.parametrize("iterations", (0, 1, 5))
def test_denoised_matches_the_host_lane_code(name, iterations):
    r = _ready(name, 64, 48, 8)
    r.denoise_iterations = iterations
    r.denoise()
    got = r.denoised()
    ref = _host(r)
    assert np.array_equal(_bits(got), _bits(ref)), (name, iterations, int((_bits(got) != _bits(ref)).any(axis=2).sum()))
    if iterations == 0:
        assert np.array_equal(_bits(got), _bits(r.framebuffer()))
    else:
        assert not np.array_equal(_bits(got), _bits(r.framebuffer()))


def test_denoised_with_other_sigmas_and_many_iterations():
    r = _ready("c1", 64, 48, 6)
    for sg, it in (((1.0, 3.0, 0.5, 0.1, 2.0), 5), ((16.0, 16.0, 0.1, 0.25, 0.2), 3), ((4.0, 0.5, 0.1, 0.25, 0.2), 10)):
        r.denoise_sigma = sg
        r.denoise_iterations = it
        r.denoise()
        assert np.array_equal(_bits(r.denoised()), _bits(_host(r))), (sg, it)


def test_denoised_on_a_ragged_frame_and_one_sample():
    r = _ready("c1", 50, 37, 5, 3)
    r.denoise()
    assert np.array_equal(_bits(r.denoised()), _bits(_host(r)))
    r.reset()
    r.render(1)                                              # n = 1: zero variance
    r.denoise()
    assert np.array_equal(_bits(r.denoised()), _bits(_host(r)))


def test_denoise_leaves_the_frame_alone_and_repeats_itself():
    r = _ready("c3", 48, 40, 8)
    r.draw()
    fb, var, feat, disp = r.framebuffer(), r.variance(), r.features(), r.display()
    r.denoise()
    first = r.denoised()
    r.denoise()
    assert np.array_equal(_bits(r.denoised()), _bits(first))
    assert np.array_equal(_bits(r.framebuffer()), _bits(fb))
    assert np.array_equal(_bits(r.variance()), _bits(var))
    assert np.array_equal(_bits(r.features()), _bits(feat))
    assert np.array_equal(_bits(r.display()), _bits(disp))
    r.draw()
    assert np.array_equal(_bits(r.display()), _bits(disp))


def test_refusals_and_recovery():
    r = scenes.hip_scene("c1", 32, 32)
    with pytest.raises(volren_amd.VolrenError, match="denoise"):
        r.denoised()                                         # before any denoise
    r.variance = 1
    r.render(4)
    with pytest.raises(volren_amd.VolrenError, match="feature pass"):
        r.denoise()                                          # no features yet
    r.render_features(4)
    r.denoise()
    r.denoised()
    r.resize(48, 32)                                         # drops features and the denoised buffer
    with pytest.raises(volren_amd.VolrenError, match="denoise"):
        r.denoised()
    r.render(4)
    with pytest.raises(volren_amd.VolrenError, match="feature pass"):
        r.denoise()
    r.render_features(4)
    r.reset()
    with pytest.raises(volren_amd.VolrenError, match="sample < 1"):
        r.denoise()
    r.variance = 0
    r.render(2)
    r.variance = 1
    r.render(2)                                              # moments switched on mid-frame
    with pytest.raises(volren_amd.VolrenError, match="moments"):
        r.denoise()
    r.reset()
    r.render(4)
    r.set_tiles([0, 2])
    with pytest.raises(volren_amd.VolrenError, match="tile subset"):
        r.denoise()
    r.set_tiles([])
    r.reset()
    r.render(4)
    r.denoise()
    assert np.array_equal(_bits(r.denoised()), _bits(_host(r)))


def test_noise_reduction_on_smoke_brick():
    """c2 (smoke.brick) at 256^2, 16 spp (features 16 spp), against 1024 spp of another seed.  Measured: raw 0.120, denoised 0.040 (ratio 0.33);
    bound 0.5."""
    ref = scenes.hip_scene("c2", 256, 256)
    ref.seed = 777
    ref.render(1024)
    want = ref.framebuffer()[..., :3]
    r = _ready("c2", 256, 256, 16)
    r.denoise()
    raw = scenes.rel_l2(r.framebuffer()[..., :3], want)
    den = scenes.rel_l2(r.denoised()[..., :3], want)
    assert den <= 0.5 * raw, (raw, den)


def test_python_and_volpy_shapes_and_row_order():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.variance = 1
    vr.render(6)
    vr.render_features(6)
    vr.denoise()
    r = vr._r
    raw = np.empty(24 * 40 * 4, np.float32)
    assert r._L.vr_denoised(r._h, raw.ctypes.data) == 0
    d = r.denoised()
    assert d.shape == (24, 40, 4) and np.array_equal(d.reshape(-1), raw)          # row 0 = bottom, like framebuffer()
    dd = vr.denoised_data()
    assert dd.shape == (40, 24, 3) == vr.fbo_data().shape
    assert np.array_equal(dd.reshape(-1), d[..., :3].reshape(-1))


def test_cli_render_denoise_writes_the_tonemapped_denoised_frame(tmp_path):
    from PIL import Image

    from oracle import binding as ob
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "12", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--denoise", "--output", "dn.png"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    img = np.asarray(Image.open(tmp_path / "dn_000000.png"))
    r = scenes.hip_scene("readme", 96, 80)
    r.variance = 1
    r.render(12)
    r.render_features(12)
    r.denoise()
    tm = r.denoised()
    ob.lib().orc_tonemap(ob.fptr(tm), 96, 80, 3.0, 2.0)
    want = np.floor(np.clip(tm[::-1], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert img.shape == (80, 96, 4) and np.array_equal(img, want)
    plain = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--output", "raw.png"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0
    assert (tmp_path / "raw_000000.png").read_bytes() != (tmp_path / "dn_000000.png").read_bytes()
    bad = subprocess.run([exe, scenes.SMOKE, scenes.HDR, "--gpus", "2"] + args + ["--denoise"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--denoise" in bad.stderr


# ---- shapes, HDR input, the limits of denoise_sigma, flush points -----------------------------------------------------------------------------------
def _same_denoised(r, what, iterations=None, sigma=None):
    if iterations is not None:
        r.denoise_iterations = iterations
    if sigma is not None:
        r.denoise_sigma = sigma
    r.denoise()
    got = r.denoised()
    ref = _host(r)
    bad = (_bits(got) != _bits(ref)).any(axis=2)
    assert not bad.any(), (what, int(bad.sum()))
    assert np.isfinite(got).all(), what
    return got


def _nontrivial(r):
    assert (r.features()[..., 3] > 0).any() and (r.variance()[..., :3] > 0).any()


@pytest.mark.parametrize("w,h", ((1, 1), (1, 37), (37, 1), (15, 9), (16, 16), (17, 16), (33, 31)))
def test_denoised_on_small_and_thin_frames(w, h):
    """frames one pixel wide or tall, narrower than a tile, one tile, one tile and a column, two tiles and a ragged row and column"""
    r = _ready("c1", w, h, 6)
    _nontrivial(r)
    for it in (0, 1, 5):
        got = _same_denoised(r, (w, h, it), it)
        if it == 0:
            assert np.array_equal(_bits(got), _bits(r.framebuffer()))
        elif w * h > 1:
            assert not np.array_equal(_bits(got), _bits(r.framebuffer()))


@pytest.mark.parametrize("w,h,it", ((1030, 770, 10), (1920, 1080, 5)))
def test_denoised_on_large_frames(w, h, it):
    """1030 x 770 at N = 10: the step-512 taps of the last iteration land inside the frame; 1920 x 1080 at N = 5"""
    r = _ready("c1", w, h, 2, 1)
    _nontrivial(r)
    got = _same_denoised(r, (w, h, it), it)
    assert not np.array_equal(_bits(got), _bits(r.framebuffer()))


def test_denoised_on_hdr_input():
    """c1 under an environment 1e4 times as strong, 2 spp"""
    r = scenes.hip_scene("c1", 48, 32)
    r.env_strength = 1e4
    r.variance = 1
    r.render(2)
    r.render_features(2)
    _nontrivial(r)
    assert r.framebuffer()[..., :3].max() > 1e3 and r.variance()[..., :3].max() > 1e6
    got = _same_denoised(r, "hdr")
    assert not np.array_equal(_bits(got), _bits(r.framebuffer()))


def test_denoised_at_the_limits_of_each_sigma():
    """Each sigma alone at the smallest and the largest value the API accepts (2^-60 and 2^60: sigma_a^2 down to 2^-120, where a device that
    flushed subnormals would still agree): finite, and the device equal to the host"""
    lo, hi = hk_denoise.sigma_range()
    r = _ready("c1", 64, 48, 8)
    _nontrivial(r)
    for i in range(5):
        for v in (lo, hi):
            sg = list(hk_denoise.DEFAULT_SIGMA)
            sg[i] = v
            _same_denoised(r, ("sigma", i, v), 5, tuple(sg))


def test_every_flush_point_sees_the_pending_samples():
    """trace() x n, then variance(), features(), render_features() or denoise(): each gives what it gives after render(n)"""
    n = 5
    ref = _ready("c1", 40, 32, n)
    ref.denoise()
    want_fb, want_var, want_feat, want_den = ref.framebuffer(), ref.variance(), ref.features(), ref.denoised()
    r = _ready("c1", 40, 32, 1, n)
    for step in ("variance", "features", "render_features", "denoise"):
        r.reset()
        for _ in range(n):
            r.trace()
        if step == "variance":
            assert np.array_equal(_bits(r.variance()), _bits(want_var))
        elif step == "features":
            assert np.array_equal(_bits(r.features()), _bits(want_feat))
        elif step == "render_features":
            r.render_features(n)
            assert np.array_equal(_bits(r.features()), _bits(want_feat))
        else:
            r.denoise()
            assert np.array_equal(_bits(r.denoised()), _bits(want_den))
        assert r.sample == n and np.array_equal(_bits(r.framebuffer()), _bits(want_fb)), step
