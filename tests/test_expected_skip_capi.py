"""CPU: the public surface of empty-space skipping in the expected-value feature pass -- vr_expected_stats and vr_expected_clear_table exported,
listed and documented, their arguments checked before the device; the settings "expected_skip" and "expected_stats" taken and range-checked (where
a renderer can exist; tests/test_gpu_expected_skip.py runs the same check on the device); the Python, volpy and command-line layers above them.
What the pass computes needs a device: tests/test_gpu_expected_skip.py."""
import ctypes as C
import inspect
import os
import subprocess

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NAMES = ("vr_expected_stats", "vr_expected_clear_table")
VR_ERR, VR_ERR_NO_DEVICE, VR_ERR_ARG = 1, 2, 3


def test_the_symbols_are_exported_listed_and_documented():
    lib = volren_amd.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in volren_amd.SYMBOLS and name in declared_functions()
    assert lib.vr_expected_stats.argtypes == [C.c_void_p, C.c_void_p] and lib.vr_expected_clear_table.argtypes == [C.c_void_p] * 3
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    at = text.index('vr_set_int "expected_skip"')
    doc = text[at:text.index("vr_features waits", at)]
    for words in ("the default", "Results never depend on the setting", "+0.0f", "Chebyshev", '"expected_stats"', "vr_expected_stats", "vr_expected_clear_table",
                  "steps that fetched", "VR_ERR", "vr_clear.h"):
        assert words in doc, words
    for header in ("vr_clear.h", "vr_expected.h"):
        assert os.path.exists(os.path.join(scenes.ROOT, "volren_amd", "csrc", header))
    assert "nothing is skipped" not in open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_expected.h")).read()


def test_null_arguments_are_refused_before_the_device():
    lib = volren_amd.load()
    fake = C.create_string_buffer(256)                              # never dereferenced: the argument checks come first
    out, cells = (C.c_uint64 * 4)(), (C.c_int * 3)()
    assert lib.vr_expected_stats(None, out) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error()
    assert lib.vr_expected_stats(C.addressof(fake), None) == VR_ERR_ARG
    assert lib.vr_expected_clear_table(None, None, cells) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error()
    assert lib.vr_expected_clear_table(C.addressof(fake), None, None) == VR_ERR_ARG
    if lib.vr_device_count() <= 0:
        assert lib.vr_expected_stats(C.addressof(fake), out) == VR_ERR_NO_DEVICE and b"no HIP device" in lib.vr_last_error()
        assert lib.vr_expected_clear_table(C.addressof(fake), None, cells) == VR_ERR_NO_DEVICE


def check_settings(r):
    """the two settings on renderer r: defaults, the values taken, the values refused (which keep the old one)"""
    lib = volren_amd.load()
    assert r.expected_skip == 1 and r.get_int("expected_stats") == 0
    for name in ("expected_skip", "expected_stats"):
        for v in (0, 1):
            setattr(r, name, v)
            assert r.get_int(name) == v
            for bad in (-1, 2, 2 ** 31 - 1):
                assert lib.vr_set_int(r._h, name.encode(), bad) == VR_ERR and name.encode() in lib.vr_last_error(), (name, bad)
                assert r.get_int(name) == v
    r.expected_stats = 0
    r.expected_skip = 1


def test_the_settings_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        r = volren_amd.Renderer(16, 16)
        check_settings(r)
        r.close()


def test_the_python_layers_carry_the_new_names():
    import volren_amd.volpy as volpy
    from volren_amd import renderer
    assert "expected_skip" in renderer._INT_FIELDS and "expected_stats" in renderer._INT_FIELDS
    assert inspect.signature(volren_amd.Renderer.expected_stats).parameters["enable"].default is None
    assert callable(volren_amd.Renderer.expected_clear_table)
    prop = volren_amd.ShardedRenderer.expected_skip
    assert isinstance(prop, property) and prop.fset is not None and "every part" in prop.__doc__
    assert "expected_skip" in volpy._PASS_THROUGH                   # read and written through volpy.Renderer
    assert "expected_skip" in volpy.Renderer.render_features_expected.__doc__


def test_the_cli_takes_the_flag_only_with_expected_features_and_only_0_or_1():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--denoise", "--expected-skip", "1"), "--expected-skip needs --expected-features"),
                         (("--expected-skip", "0"), "--expected-skip needs --expected-features"),
                         (("--denoise", "--expected-features", "2", "--expected-skip", "2"), "--expected-skip: 0 (march every step) or 1"),
                         (("--denoise", "--expected-features", "2", "--expected-skip", "-1"), "--expected-skip: 0 (march every step) or 1"),
                         (("--denoise", "--expected-features", "2", "--expected-skip"), "missing value after --expected-skip")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
