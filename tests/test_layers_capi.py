"""CPU: the public surface of the layered filter -- vr_denoised_layer exported, listed and documented, its arguments checked before the device, the call
failing loudly without one; the setting "denoise_layers" taken and range-checked (where a renderer can exist; tests/test_gpu_layers.py runs the same
check, and every refusal, on the device); the Python, volpy and command-line layers above them.  What the call computes: tests/test_layers_host.py on
the host build, tests/test_gpu_layers.py on the device."""
import ctypes as C
import os
import subprocess

import scenes
import volren_amd
from test_capi_symbols import declared_functions

VR_ERR, VR_ERR_NO_DEVICE, VR_ERR_ARG = 1, 2, 3


def test_the_symbol_is_exported_listed_and_documented():
    lib = volren_amd.load()
    assert hasattr(lib, "vr_denoised_layer") and "vr_denoised_layer" in volren_amd.SYMBOLS and "vr_denoised_layer" in declared_functions()
    assert lib.vr_denoised_layer.argtypes == [C.c_void_p] * 2
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    at = text.index("the filter on the scattered layer alone")
    doc = text[at:text.index("int vr_denoised_layer(", at)]
    for words in ('"denoise_layers"', "default 0", "drops the history", "G = (1 - kappa) B", "S.rgb = y.rgb - G", "F.a > 2^-20", "kappa / F.a", "max(0, G + L.rgb)",
                  "whatever \"denoise_resolve\" says", "the frame's variance", "holds the layer", "rays >= 2", "0.0004", "loses", "vr_sharded_denoise", "vr_layers.h",
                  "(1 - a) B' + rgb", "VR_ERR", "bit for bit"):
        assert words in doc, words
    header = open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_layers.h")).read()
    for words in ("S_p.rgb = y_p.rgb - G_p", "F_p.a > 2^-20", "max_(G_p + L_p.rgb, 0)", "bit for bit", "0.0004"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md"):
        body = open(os.path.join(scenes.ROOT, doc)).read()
        assert "denoise_layers" in body and "vr_layers.h" in body, doc


def test_null_arguments_are_refused_before_the_device_and_the_call_fails_loudly_without_one():
    lib = volren_amd.load()
    out = (C.c_float * 4)()
    fn = lib.vr_denoised_layer
    assert fn(None, out) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error()
    assert fn(C.c_void_p(1), None) == VR_ERR_ARG                      # (the handle is not touched before the argument check ...
    if lib.vr_device_count() <= 0:
        assert fn(C.c_void_p(1), out) == VR_ERR_NO_DEVICE and b"no HIP device" in lib.vr_last_error()      # ... nor before the device check)


def check_setting(r):
    """"denoise_layers" on renderer r: the default, the values taken, the values refused (which keep the old one)"""
    lib = volren_amd.load()
    assert r.get_int("denoise_layers") == 0
    for v in (1, 0):
        r.denoise_layers = v
        assert r.get_int("denoise_layers") == v and r.denoise_layers == v
        for bad in (-1, 2, 2 ** 31 - 1):
            assert lib.vr_set_int(r._h, b"denoise_layers", bad) == VR_ERR and b"denoise_layers" in lib.vr_last_error(), bad
            assert r.get_int("denoise_layers") == v


def test_the_setting_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        r = volren_amd.Renderer(16, 16)
        check_setting(r)
        r.close()


def test_the_python_layers_carry_the_new_names():
    import volren_amd.volpy as volpy
    from volren_amd import renderer
    assert "denoise_layers" in renderer._INT_FIELDS
    assert callable(volren_amd.Renderer.denoised_layer) and "premultiplied" in volren_amd.Renderer.denoised_layer.__doc__
    prop = volren_amd.ShardedRenderer.denoise_layers
    assert isinstance(prop, property) and prop.fset is not None and "part 0" in prop.__doc__
    assert callable(volren_amd.ShardedRenderer.denoised_layer)
    assert callable(volpy.Renderer.denoised_layer_data) and "fbo_data()'s shape" in volpy.Renderer.denoised_layer_data.__doc__
    assert "denoise_layers" in volpy._PASS_THROUGH                         # read and written through volpy.Renderer


def test_the_cli_takes_the_flag_only_with_a_filter_and_two_or_more_expected_rays():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--denoise-layers",), "--denoise-layers needs --denoise or --denoise-temporal"),
                         (("--denoise-layers", "--resolve", "--expected-features", "2"), "--denoise-layers needs --denoise or --denoise-temporal"),
                         (("--denoise", "--denoise-layers"), "--denoise-layers needs --expected-features N with N >= 2"),
                         (("--denoise-temporal", "--denoise-layers", "--expected-features", "1"), "--denoise-layers needs --expected-features N with N >= 2"),
                         (("--denoise", "--denoise-layers", "--expected-features", "2", "--gpus", "2"), "renders on one device only")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
