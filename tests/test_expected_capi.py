"""CPU: the C ABI of the expected-value feature pass (vr_render_features_expected, vr_sharded_render_features_expected) -- exported, listed,
documented, its arguments checked before the device and failing loudly without one -- and the Python and command-line layers above it.  What the
pass computes needs a device: tests/test_gpu_expected.py."""
import ctypes as C
import os
import subprocess

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NAMES = ("vr_render_features_expected", "vr_sharded_render_features_expected")
VR_ERR_NO_DEVICE, VR_ERR_ARG = 2, 3


def test_both_symbols_are_exported_listed_and_documented():
    lib = volren_amd.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in volren_amd.SYMBOLS and name in declared_functions()
        assert getattr(lib, name).argtypes == [C.c_void_p, C.c_int]
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    at = text.index("vr_render_features_expected fills the same buffer")
    doc = text[at:text.index("vr_features waits", at)]
    for words in ("rays in 1..4", "VR_ERR_ARG", "T <= 2^-10", "Asynchronous", "flush point", "vr_expected.h"):
        assert words in doc, words
    assert os.path.exists(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_expected.h"))


def test_null_handles_and_rays_out_of_range_are_refused_before_the_device():
    lib = volren_amd.load()
    fake = C.create_string_buffer(256)                              # never dereferenced: the argument checks come first
    for name, words in zip(NAMES, (b"null renderer", b"null sharded renderer")):
        fn = getattr(lib, name)
        assert fn(None, 2) == VR_ERR_ARG and words in lib.vr_last_error()
        for rays in (0, 5, -1):
            assert fn(C.addressof(fake), rays) == VR_ERR_ARG, (name, rays)
            assert b"rays must be 1..4" in lib.vr_last_error()


def test_without_a_device_the_call_fails_loudly():
    lib = volren_amd.load()
    if lib.vr_device_count() > 0:
        return                                                      # with a device the call runs: tests/test_gpu_expected.py
    fake = C.create_string_buffer(256)
    for rays in (1, 2, 4):
        assert lib.vr_render_features_expected(C.addressof(fake), rays) == VR_ERR_NO_DEVICE and b"no HIP device" in lib.vr_last_error()


def test_the_python_layers_have_the_method():
    import inspect

    import volren_amd.volpy as volpy
    for cls in (volren_amd.Renderer, volren_amd.ShardedRenderer):
        sig = inspect.signature(cls.render_features_expected)
        assert sig.parameters["rays"].default == 2 and sig.parameters["sync"].default is True
    assert inspect.signature(volpy.Renderer.render_features_expected).parameters["rays"].default == 2


def test_the_cli_refuses_the_flag_without_a_denoise_flag_and_a_count_out_of_range():
    """both refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--expected-features", "2"), "--expected-features needs --denoise"),
                         (("--denoise-moments", "--expected-features", "2"), "needs --denoise"),
                         (("--denoise", "--expected-features", "5"), "must be 1..4"),
                         (("--denoise-temporal", "--expected-features", "0"), "must be 1..4"),
                         (("--denoise", "--expected-features"), "missing value after --expected-features")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
