"""GPU: the layered filter ("denoise_layers" = 1: vr_filters.hip layers_split_kernel and layers_merge_kernel around the denoiser's own kernels,
vr_denoised_layer) bit for bit against the host composition of the same headers (tests/hk_layers.py on tests/hostkernel/layers_host.cpp, itself held to a
float64 statement by tests/test_layers_host.py), on frames with partial tiles; vr_denoise_temporal with rejection and with moments against the host chain;
the setting at 0 against a renderer that never saw it; every refusal on a live renderer; a ragged frame; the sharded renderer; the volpy and
command-line layers."""
import subprocess

import numpy as np
import pytest

import hk_adaptive as ha
import hk_layers as hl
import hk_resolve as hr
import scenes
import volren_amd
from gpu_frames import _camera, _orbit
from hk_common import same as _same
from test_gpu_resolve import _frame, _pair
from test_layers_capi import check_setting

pytestmark = pytest.mark.gpu

W, H, SPP, RAYS = 64, 48, 4, 2                  # 4 x 3 tiles
SCENES = ("c2", "c3env", "c3", "c4_64")          # smoke.brick in front of the sky; under the LUT with the sky shown; under the LUT as configured (sky hidden); dense fp16


def _host(r, o):
    """the host composition on the renderer's own buffers: (out, L, y, S)"""
    fb, guide = r.framebuffer(), r.features()
    y, B = hr.resolved(o, RAYS, fb, guide)
    out, L, S, _ = hl.layered(y, B, r.variance(), guide, r.sample, r.denoise_iterations, tuple(r.denoise_sigma))
    return out, L, y, S


@pytest.mark.parametrize("name", SCENES)
def test_split_merge_and_the_whole_call_match_the_host_bit_for_bit(name):
    """a 64x48 frame of 4 spp against 2 x 2 expected rays: vr_denoised and vr_denoised_layer after vr_denoise; with zero iterations the merge of the split alone;
    the first vr_denoise_temporal's history is the split's S.  The framebuffer, the features and vr_resolved are left as they were."""
    r, o = _pair(name, W, H)
    r.variance = 1
    _frame(r)
    r.denoise()
    parent = r.denoised()
    r.resolve()
    fb, guide, y = r.framebuffer(), r.features(), r.resolved()
    r.denoise_layers = 1
    r.denoise()
    out, L, want_y, S = _host(r, o)
    assert _same(r.denoised(), out) and _same(r.denoised_layer(), L)
    assert _same(r.framebuffer(), fb) and _same(r.features(), guide) and _same(r.resolved(), y) and _same(y, want_y)
    assert not _same(out, parent) and _same(out[..., 3], guide[..., 3]) and _same(L[..., 3], guide[..., 3])
    none = guide[..., 3] == 0
    assert none.sum() > 100 or name == "c4_64"
    assert _same(out[none][:, :3], r.resolve_background()[none][:, :3])      # the sky around the volume is B itself
    r.denoise_iterations = 0
    r.denoise()
    out0, L0, _, _ = _host(r, o)
    assert _same(r.denoised(), out0) and _same(r.denoised_layer(), L0) and _same(L0[..., :3], S[..., :3])
    r.denoise_iterations = 5
    r.denoise_temporal()
    assert _same(r.denoise_history()[0], S) and _same(r.denoised(), out)
    r.close()


# thin both ways, one pixel past a tile, one short of two tiles
@pytest.mark.parametrize("w,h", ((1, 37), (37, 1), (17, 16), (33, 31)))
def test_thin_and_one_past_a_tile_frames_match_the_host_bit_for_bit(w, h):
    r, o = _pair("c2", w, h)
    r.variance = 1
    r.denoise_layers = 1
    _frame(r, spp=2)
    r.denoise()
    out, L, _, _ = _host(r, o)
    assert _same(r.denoised(), out) and _same(r.denoised_layer(), L)
    r.close()


@pytest.mark.parametrize("turn", (0.0, 1.0))
@pytest.mark.parametrize("setting,value", (("denoise_reject", 3.0), ("denoise_moments", 1)))
def test_three_temporal_frames_match_the_host_chain(setting, value, turn):
    """c3env, three frames of 4 spp, the camera fixed or turned 1 degree per frame about the volume: history (which holds the layer), result and layer"""
    r, o = _pair("c3env", W, H)
    r.variance = 1
    r.denoise_layers = 1
    setattr(r, setting, value)
    replay = hl.Replay(moments=setting == "denoise_moments")
    for i in range(3):
        for x in (r, o):
            _orbit(x, turn * i)
        _frame(r, seed=100 + i)
        r.denoise_temporal()
        fb, guide = r.framebuffer(), r.features()
        y, B = hr.resolved(o, RAYS, fb, guide)
        want = replay.frame(_camera(r), y, B, r.variance(), guide, r.sample, r.denoise_alpha, r.denoise_iterations, tuple(r.denoise_sigma),
                            tau=r.denoise_reject)
        hc, hv, hn = r.denoise_history()
        for got, ref, part in ((hc, want[0], "C"), (hv, want[1], "V"), (hn, want[2], "N"), (r.denoised(), want[3], "denoised"), (r.denoised_layer(), want[4], "L")):
            assert _same(got, ref), (setting, turn, i, part)
        if i == 0:
            assert _same(hc, hl.split(y, B, guide[..., 3])) and not _same(hc, y)
    assert (hn == 3).mean() > 0.5                    # (the rejection restarts some pixels, the turn brings others into the frame)
    r.close()


def test_the_setting_at_0_is_a_renderer_that_never_heard_of_it():
    """denoised, the history and the framebuffer after the setting went 1 and back to 0, against a fresh renderer's"""
    a, _ = _pair("c3env", W, H)
    b, _ = _pair("c3env", W, H)
    for r in (a, b):
        r.variance = 1
    _frame(b)
    b.denoise_layers = 1
    b.denoise()
    b.denoise_temporal()
    b.denoise_layers = 0
    with pytest.raises(volren_amd.VolrenError, match="no history"):      # the change dropped it
        b.denoise_history()
    for r in (a, b):
        _frame(r, seed=7)
        r.denoise()
    assert _same(a.denoised(), b.denoised()) and _same(a.framebuffer(), b.framebuffer())
    for i in range(2):
        for r in (a, b):
            _frame(r, seed=8 + i)
            r.denoise_temporal()
        assert _same(a.denoised(), b.denoised()) and _same(a.framebuffer(), b.framebuffer())
        for x, y in zip(a.denoise_history(), b.denoise_history()):
            assert _same(x, y)
    with pytest.raises(volren_amd.VolrenError, match="denoise_layers = 1"):
        a.denoised_layer()
    a.close()
    b.close()


def test_every_refusal_on_a_live_renderer():
    """no expected pass, one ray, stochastic features last, a tile subset, integrator 2, no samples, the values 2 and -1, vr_denoised_layer before a call --
    each VR_ERR with its reason, before a launch: the last result stays.  A change of the value drops the history."""
    r, _ = _pair("c3env", 48, 40)
    check_setting(r)
    r.variance = 1
    r.denoise_layers = 1
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1 since the last resize"):
        r.denoised_layer()
    r.reset()
    r.render(SPP)

    def refused(words):
        for call in (r.denoise, r.denoise_temporal):
            with pytest.raises(volren_amd.VolrenError, match=words):
                call()

    refused("no feature pass")
    r.render_features_expected(2)
    r.reset()
    refused("holds no samples")
    _frame(r)
    r.denoise()
    good, layer = r.denoised(), r.denoised_layer()
    r.render_features(4)
    refused("denoise_layers = 1: the feature buffer was not last filled by render_features_expected")
    r.render_features_expected(1)
    refused("denoise_layers = 1: the expected-value pass ran with rays = 1; rays >= 2 is needed")
    r.render_features_expected(2)
    r.set_tiles([0, 1])
    refused("tile subset")
    r.set_tiles([])
    r.integrator = 2
    refused("denoise_layers = 1: integrator = 2")
    r.integrator = 0
    assert _same(r.denoised(), good) and _same(r.denoised_layer(), layer)
    r.denoise_temporal()
    assert (r.denoise_history()[2] == 1).all()
    r.denoise_layers = 0
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    r.denoise_temporal()
    r.denoise_layers = 1
    with pytest.raises(volren_amd.VolrenError, match="no history"):
        r.denoise_history()
    r.resize(40, 24)
    with pytest.raises(volren_amd.VolrenError, match="no denoise with denoise_layers = 1 since the last resize"):
        r.denoised_layer()
    r.close()


def test_a_ragged_adaptive_frame():
    r, o = _pair("c2", 48, 40)
    r.denoise_layers = 1
    r.render_adaptive(2, 16, 0.05)
    counts = r.tile_samples()
    assert len(set(counts.reshape(-1).tolist())) > 1
    r.render_features_expected(2)
    r.denoise()
    fb, guide = r.framebuffer(), r.features()
    y, B = hr.resolved(o, 2, fb, guide)
    out, L, _, _ = hl.layered(y, B, r.variance(), guide, ha.per_pixel(counts, 48, 40), r.denoise_iterations, tuple(r.denoise_sigma))
    assert _same(r.denoised(), out) and _same(r.denoised_layer(), L)
    r.close()


def test_two_logical_shards_equal_one_device():
    from test_gpu_resolve import _configure
    name, w, h = "c3env", 96, 64
    one, _ = _pair(name, w, h)
    one.variance = 1
    one.denoise_layers = 1
    _frame(one)
    one.denoise()
    spatial, layer = one.denoised(), one.denoised_layer()
    one.denoise_temporal()
    s = volren_amd.ShardedRenderer(w, h, [0, 0])
    s.each(lambda p: _configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    assert s.denoise_layers == 0
    s.denoise_layers = 1
    assert s.denoise_layers == 1 and all(p.denoise_layers == 1 for p in s.parts)
    s.render(SPP)
    s.render_features(2)
    with pytest.raises(volren_amd.VolrenError, match="denoise_layers = 1: the feature buffer was not last filled by render_features_expected"):
        s.denoise()
    s.render_features_expected(RAYS)
    s.denoise()
    assert _same(s.framebuffer(), one.framebuffer()) and _same(s.features(), one.features())
    assert _same(s.denoised(), spatial) and _same(s.denoised_layer(), layer)
    s.denoise_temporal()
    assert _same(s.denoised(), one.denoised()) and _same(s.denoised_layer(), one.denoised_layer())
    s.close()
    one.close()


def test_volpy_has_the_names():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.cam_fov = 40.0
    vr.variance = 1
    vr.render(4)
    vr.render_features_expected(2)
    vr.denoise()
    plain = vr.denoised_data()
    assert vr.denoise_layers == 0
    vr.denoise_layers = 1
    assert vr.denoise_layers == 1 and vr._r.denoise_layers == 1
    vr.denoise()
    layer = vr.denoised_layer_data()
    assert layer.shape == (40, 24, 4) and np.array_equal(layer.reshape(-1), vr._r.denoised_layer().reshape(-1))
    assert not np.array_equal(vr.denoised_data(), plain)


def test_cli_flag_changes_the_file_and_is_refused_alone(tmp_path):
    from PIL import Image

    from oracle import binding as ob
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "6", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    r = scenes.hip_scene("readme", 96, 80)
    r.variance = 1
    r.render(6)
    r.render_features_expected(2)
    images = []
    for flags, layers in ((["--denoise"], 0), (["--denoise", "--denoise-layers"], 1)):
        r.denoise_layers = layers
        r.denoise()
        out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + flags + ["--expected-features", "2", "--output", "ly.png"], cwd=tmp_path,
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        img = np.asarray(Image.open(tmp_path / "ly_000000.png"))
        tm = r.denoised()
        ob.lib().orc_tonemap(ob.fptr(tm), 96, 80, 3.0, 2.0)
        want = np.floor(np.clip(tm[::-1], 0, 1) * 255.0 + 0.5).astype(np.uint8)
        assert img.shape == (80, 96, 4) and np.array_equal(img, want), flags
        images.append(img.copy())
    assert not np.array_equal(images[0], images[1])
    out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--denoise-layers", "--output", "no.png"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "--denoise-layers needs --denoise or --denoise-temporal" in out.stderr
    r.close()
