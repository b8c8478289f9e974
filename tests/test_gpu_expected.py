"""GPU: the expected-value feature pass (vr_render_features_expected, vr_launch.hip features_expected_kernel) bit for bit against the host build of
the same header (tests/hostkernel/expected_host.cpp, itself held to a float64 statement by tests/test_expected_host.py), on every grid form, on
partial tiles, tile subsets and cameras at the edge of its domain; and everything that reads the feature buffer reading it unchanged: vr_features,
the filter, the temporal accumulation, the sharded renderer and the command line."""
import subprocess

import numpy as np
import pytest

import hk_denoise
import hk_expected as he
import scenes
import volren_amd
from hk_common import bits as _bits
from hk_common import same as _same

pytestmark = pytest.mark.gpu

SHAPES = ((64, 48), (50, 38), (16, 1))          # whole tiles; partial tiles on both edges; a single row
RAYS = (1, 2, 3)


def _pair(name, w, h):
    return scenes.hip_scene(name, w, h), scenes.oracle_scene(name, w, h)


def _same_expected(r, o, rays, what):
    r.render_features_expected(rays)
    got, ref = r.features(), he.expected_pass(o, rays)
    bad = (_bits(got) != _bits(ref)).any(axis=2)
    assert not bad.any(), (what, rays, int(bad.sum()))
    return got


@pytest.mark.parametrize("name", ("c1", "c3", "c4_64", "c5_64"))
def test_the_kernel_matches_the_host_build_bit_for_bit(name):
    """smoke.brick, + lut.txt, a dense fp16 grid, brick grids with an emission grid (which plays no part), at 64x48, 50x38 and 16x1 with 1, 2 and 3
    rays per axis"""
    r, o = _pair(name, *SHAPES[0])
    for w, h in SHAPES:
        r.resize(w, h)
        o.resize(w, h)
        for rays in RAYS:
            got = _same_expected(r, o, rays, (name, w, h))
            if h > 1:
                assert (got[..., 3] > 0).any() and (np.abs(got[..., 4:7]).sum(axis=2) > 0).any() and not (got[..., 3] > 0).all()
    r.close()


def _inside(x):
    x.cam_pos, x.cam_dir, x.cam_fov = (0.05, 0.0, -0.1), (0.4, 0.2, 1.0), 80.0


def _away(x):
    x.cam_dir = tuple(-float(v) for v in x.cam_dir)


def _far(x):
    x.cam_pos, x.cam_fov = tuple(36000.0 * float(v) for v in x.cam_pos), 40.0 / 36000.0


def _crop(x):
    x.vol_clip_min, x.vol_clip_max = (0.1, 0.2, 0.0), (0.8, 0.9, 0.7)


@pytest.mark.parametrize("case", (_inside, _away, _far, _crop), ids=lambda f: f.__name__[1:])
def test_cameras_and_crops_at_the_edge(case):
    r, o = _pair("c3" if case is _crop else "c1", 40, 30)
    for x in (r, o):
        case(x)
    got = _same_expected(r, o, 2, case.__name__)
    assert np.isfinite(got).all()
    if case is _away:
        assert not got.any()
    elif case is not _far:
        assert (got[..., 3] > 0).any()
    r.close()


def test_a_tile_subset_leaves_the_other_pixels_alone():
    r, o = _pair("c1", 48, 40)                  # 3 x 3 tiles, the top row partial
    r.render_features(1)                        # the other pass fills the buffer first: both write the same one
    before = r.features()
    tiles = [1, 3, 7]
    r.set_tiles(tiles)
    r.render_features_expected(2)
    after, ref = r.features(), he.expected_pass(o, 2)
    mask = np.zeros((40, 48), bool)
    for t in tiles:
        ty, tx = divmod(t, 3)
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    assert _same(after[mask], ref[mask]) and (ref[mask][:, 3] > 0).any()
    assert _same(after[~mask], before[~mask]) and not _same(before[mask], ref[mask])
    r.close()


def test_it_counts_as_a_feature_pass_and_bad_counts_are_refused():
    r = scenes.hip_scene("c1", 16, 16)
    with pytest.raises(volren_amd.VolrenError):
        r.features()
    for rays in (0, 5, -1):
        with pytest.raises(volren_amd.VolrenError, match="rays must be 1..4"):
            r.render_features_expected(rays)
    r.render_features_expected(4)
    assert (r.features()[..., 3] > 0).any()
    r.resize(24, 16)
    with pytest.raises(volren_amd.VolrenError, match="render_features"):
        r.features()
    r.close()


def test_the_filter_and_the_temporal_accumulation_read_it_unchanged():
    """after render(16) with variance = 1: denoise() on the expected guide is the host filter on the same inputs, bit for bit; and four frames of a
    fixed camera, the guide rendered afresh for each, leave every pixel with a history of length 4"""
    r, o = _pair("c1", 64, 48)
    r.variance = 1
    r.render(16)
    r.render_features_expected(2)
    guide = r.features()
    assert _same(guide, he.expected_pass(o, 2))
    r.denoise()
    want = hk_denoise.denoise(r.framebuffer(), r.variance(), guide, r.sample, r.denoise_iterations, tuple(r.denoise_sigma))
    assert _same(r.denoised(), want) and not _same(want, r.framebuffer())
    for i in range(4):
        r.seed = 100 + i
        r.reset()
        r.render(2)
        r.render_features_expected(2)
        r.denoise_temporal()
        assert _same(r.features(), guide)
        assert (r.denoise_history()[2] == i + 1).all(), i
    r.close()


@pytest.mark.parametrize("parts", (2, 3))
def test_logical_shards_equal_the_single_device_result(parts):
    name, w, h, spp = ("c3", 96, 64, 4) if parts == 2 else ("c1", 150, 90, 3)
    one = scenes.hip_scene(name, w, h)
    one.variance = 1
    one.render(spp)
    one.render_features_expected(2)
    one.denoise()
    assert _same(one.features(), he.expected_pass(scenes.oracle_scene(name, w, h), 2))
    s = volren_amd.ShardedRenderer(w, h, [0] * parts)
    s.each(lambda p: scenes.configure(p, name, False))

    def variance_on(p):
        p.variance = 1
    s.each(variance_on)
    s.render(spp)
    s.render_features_expected(2)
    s.denoise()
    assert _same(s.features(), one.features()) and _same(s.denoised(), one.denoised()) and _same(s.framebuffer(), one.framebuffer())
    with pytest.raises(volren_amd.VolrenError, match="rays must be 1..4"):
        s.render_features_expected(5)
    s.close()
    one.close()


def test_volpy_has_the_call():
    import volren_amd.volpy as volpy
    vr = volpy.Renderer(40, 24)
    vr.volume = volpy.Volume(scenes.SMOKE)
    vr.environment = volpy.Environment(scenes.HDR)
    vr.scale_and_move_to_unit_cube()
    vr.commit()
    vr.cam_fov = 40.0
    vr.render_features_expected()
    two = vr.feature_data().copy()
    vr._r.render_features_expected(2)
    assert two.shape == (40, 24, 8) and np.array_equal(two.reshape(-1), vr._r.features().reshape(-1)) and (two[..., 3] > 0).any()


def test_cli_render_denoise_with_the_expected_guide_writes_the_frame(tmp_path):
    from PIL import Image

    from oracle import binding as ob
    exe = scenes.ROOT + "/volren_amd/volren"
    args = ["-w", "96", "-h", "80", "--render", "--spp", "12", "--bounces", "128", "--albedo", "0.8", "--phase", "0.3", "--density", "100",
            "--env_strength", "3", "--env_rot", "270", "--exposure", "3", "--gamma", "2.0", "--cam_fov", "40"]
    out = subprocess.run([exe, scenes.SMOKE, scenes.HDR] + args + ["--denoise", "--expected-features", "2", "--output", "ex.png"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    img = np.asarray(Image.open(tmp_path / "ex_000000.png"))
    r = scenes.hip_scene("readme", 96, 80)
    r.variance = 1
    r.render(12)
    r.render_features_expected(2)
    r.denoise()
    tm = r.denoised()
    ob.lib().orc_tonemap(ob.fptr(tm), 96, 80, 3.0, 2.0)
    want = np.floor(np.clip(tm[::-1], 0, 1) * 255.0 + 0.5).astype(np.uint8)
    assert img.shape == (80, 96, 4) and np.array_equal(img, want)
    r.close()
