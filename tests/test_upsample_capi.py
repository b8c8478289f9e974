"""CPU: the public surface of the upsampling of the scattered layer -- vr_upsample and its four read-backs exported, listed and documented, their arguments
checked before the device, the calls failing loudly without one; the Python, volpy and command-line layers above them.  What the call computes:
tests/test_upsample_host.py on the host build, tests/test_gpu_upsample.py on the device."""
import ctypes as C
import os
import subprocess

import scenes
import volren_amd
from test_capi_symbols import declared_functions

VR_ERR, VR_ERR_NO_DEVICE, VR_ERR_ARG = 1, 2, 3
NAMES = ("vr_upsample", "vr_upsampled", "vr_upsampled_layer", "vr_upsampled_features", "vr_upsampled_size")


def test_the_symbols_are_exported_listed_and_documented():
    lib = volren_amd.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in volren_amd.SYMBOLS and name in declared_functions(), name
    assert lib.vr_upsample.argtypes == [C.c_void_p, C.c_int, C.c_int]
    for name in NAMES[1:]:
        assert getattr(lib, name).argtypes == [C.c_void_p] * 2, name
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    at = text.index("upsampled under a full-resolution guide")
    assert "(no reference counterpart)" in text[at - 200:at + 200]
    doc = text[at:text.index("int vr_upsampled_size(", at)]
    for words in ('"denoise_layers" = 1', "factor^2 times the spp", "cubic B-spline", "w_n w_d w_a", '"denoise_sigma"', "no coverage weight", "2^-20", "kappa_p C",
                  "max(0, (1 - kappa_p) B_p + L_p.rgb)", "B_p bit for bit", "vr_upsample.h", "flush point", "VR_ERR_ARG", "2..4", "1..4", "tile subset", "vr_resize drops them",
                  "another factor", "as they were at the denoise", "no history at the hi size", "vr_sharded_part(s, 0)", "device's work", "lose",
                  '"expected_skip"', '"expected_stats"', "W*H*8", "(1 - a) B' + rgb"):
        assert words in doc, words
    header = open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_upsample.h")).read()
    for words in ("2x + 1 - f = 2f x0 + r", "(3 a^3 - 6 a^2 + 4) / 6", "N_e += (s e) L_q.rgb", "D_e > 2^-20", "L_p.rgb = kappa_p * C", "max_(G_p + L_p.rgb, 0)", "bit for bit"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md"):
        body = open(os.path.join(scenes.ROOT, doc)).read()
        assert "vr_upsample" in body and "vr_upsample.h" in body, doc


def test_arguments_are_refused_before_the_device_and_the_calls_fail_loudly_without_one():
    lib = volren_amd.load()
    out, wh, handle = (C.c_float * 8)(), (C.c_int * 2)(), C.c_void_p(1)      # (the handle is not touched before the argument and device checks)
    assert lib.vr_upsample(None, 2, 2) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error()
    for factor, rays in ((1, 2), (5, 2), (0, 2), (-2, 2), (2 ** 31 - 1, 2)):
        assert lib.vr_upsample(handle, factor, rays) == VR_ERR_ARG and b"factor must be 2..4" in lib.vr_last_error(), factor
    for rays in (0, 5, -1):
        assert lib.vr_upsample(handle, 2, rays) == VR_ERR_ARG and b"rays must be 1..4" in lib.vr_last_error(), rays
    for name, arg in (("vr_upsampled", out), ("vr_upsampled_layer", out), ("vr_upsampled_features", out), ("vr_upsampled_size", wh)):
        fn = getattr(lib, name)
        assert fn(None, arg) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error(), name
        assert fn(handle, None) == VR_ERR_ARG, name
    if lib.vr_device_count() <= 0:
        for f in (2, 3, 4):
            assert lib.vr_upsample(handle, f, 1) == VR_ERR_NO_DEVICE and b"no HIP device" in lib.vr_last_error()
        for name, arg in (("vr_upsampled", out), ("vr_upsampled_layer", out), ("vr_upsampled_features", out), ("vr_upsampled_size", wh)):
            assert getattr(lib, name)(handle, arg) == VR_ERR_NO_DEVICE and b"no HIP device" in lib.vr_last_error(), name


def test_the_python_layers_carry_the_new_names():
    import inspect

    import volren_amd.volpy as volpy
    R = volren_amd.Renderer
    sig = inspect.signature(R.upsample)
    assert sig.parameters["factor"].default == 2 and sig.parameters["rays"].default == 2 and "denoise_layers = 1" in R.upsample.__doc__
    for name in ("upsampled", "upsampled_layer", "upsampled_features", "upsampled_size"):
        assert callable(getattr(R, name)) and getattr(R, name).__doc__, name
    sig = inspect.signature(volpy.Renderer.upsample)
    assert sig.parameters["factor"].default == 2 and sig.parameters["rays"].default == 2
    assert callable(volpy.Renderer.upsampled_data) and "fbo_data()'s shape" in volpy.Renderer.upsampled_data.__doc__


def test_the_cli_takes_the_flag_only_with_the_layered_filter():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--upsample", "2"), "--upsample needs --denoise-layers"),
                         (("--upsample", "2", "--denoise", "--expected-features", "2"), "--upsample needs --denoise-layers"),
                         (("--upsample", "2", "--denoise-layers"), "--denoise-layers needs --denoise or --denoise-temporal"),
                         (("--upsample", "2", "--denoise", "--denoise-layers"), "--denoise-layers needs --expected-features N with N >= 2"),
                         (("--upsample", "1", "--denoise", "--denoise-layers", "--expected-features", "2"), "--upsample: the factor per axis must be 2..4"),
                         (("--upsample", "5", "--denoise", "--denoise-layers", "--expected-features", "2"), "--upsample: the factor per axis must be 2..4"),
                         (("--denoise", "--denoise-layers", "--expected-features", "2", "--upsample"), "missing value after --upsample")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
