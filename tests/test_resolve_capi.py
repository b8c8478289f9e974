"""CPU: the public surface of the control variate on the expected coverage -- vr_resolve, vr_resolved and vr_resolve_background exported, listed and
documented, their arguments checked before the device, the call failing loudly without one; the setting "denoise_resolve" taken and range-checked
(where a renderer can exist; tests/test_gpu_resolve.py runs the same check, and every refusal, on the device); the Python, volpy and command-line layers
above them.  What the call computes: tests/test_resolve_host.py on the host build, tests/test_gpu_resolve.py on the device."""
import ctypes as C
import os
import subprocess

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NAMES = ("vr_resolve", "vr_resolved", "vr_resolve_background")
VR_ERR, VR_ERR_NO_DEVICE, VR_ERR_ARG = 1, 2, 3


def test_the_symbols_are_exported_listed_and_documented():
    lib = volren_amd.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in volren_amd.SYMBOLS and name in declared_functions()
    assert lib.vr_resolve.argtypes == [C.c_void_p] and lib.vr_resolved.argtypes == lib.vr_resolve_background.argtypes == [C.c_void_p] * 2
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    at = text.index("a control variate in image space")
    doc = text[at:text.index("int vr_resolve(", at)]
    for words in ("y = x + beta (kappa^ - kappa)", "beta = B - C~", "E[y] = E[x] + beta (E[kappa^] - kappa)", "stochastic-tricubic", "0.002", "emission grid",
                  "a flush point like vr_denoise", "no sample is in the frame", "tile subset", '"integrator" is 2', "vr_render_features_expected", "rays < 2",
                  '"denoise_resolve"', "default 0", "drops the history", "the frame's variance unchanged", "vr_sharded_denoise", "vr_resolve.h", "VR_ERR",
                  "ragged", "vr_resize"):
        assert words in doc, words
    header = open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_resolve.h")).read()
    for words in ("E[y] = E[x] + beta (E[kappa^] - kappa)", "stochastic-tricubic", "emission grid", "dy outer, dx inner", "bit for bit"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md"):
        assert "vr_resolve" in open(os.path.join(scenes.ROOT, doc)).read(), doc


def test_null_arguments_are_refused_before_the_device_and_the_call_fails_loudly_without_one():
    lib = volren_amd.load()
    out = (C.c_float * 4)()
    assert lib.vr_resolve(None) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error()
    for fn in (lib.vr_resolved, lib.vr_resolve_background):
        assert fn(None, out) == VR_ERR_ARG and b"null renderer" in lib.vr_last_error()
        assert fn(C.c_void_p(1), None) == VR_ERR_ARG                  # (the handle is not touched before the argument check ...
        if lib.vr_device_count() <= 0:
            assert fn(C.c_void_p(1), out) == VR_ERR_NO_DEVICE and b"no HIP device" in lib.vr_last_error()      # ... nor before the device check)
    if lib.vr_device_count() <= 0:
        try:                                                          # vr_resolve itself needs a renderer, and none can be made
            volren_amd.Renderer(16, 16)
        except volren_amd.VolrenError as e:
            assert "no HIP device" in str(e)
        else:
            raise AssertionError("a renderer without a device")


def check_setting(r):
    """"denoise_resolve" on renderer r: the default, the values taken, the values refused (which keep the old one)"""
    lib = volren_amd.load()
    for name in ("denoise_resolve",):
        assert r.get_int(name) == 0
        for v in (1, 0):
            setattr(r, name, v)
            assert r.get_int(name) == v and getattr(r, name) == v
            for bad in (-1, 2, 2 ** 31 - 1):
                assert lib.vr_set_int(r._h, name.encode(), bad) == VR_ERR and name.encode() in lib.vr_last_error(), (name, bad)
                assert r.get_int(name) == v


def test_the_setting_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        r = volren_amd.Renderer(16, 16)
        check_setting(r)
        r.close()


def test_the_python_layers_carry_the_new_names():
    import volren_amd.volpy as volpy
    from volren_amd import renderer
    assert "denoise_resolve" in renderer._INT_FIELDS
    for name in ("resolve", "resolved", "resolve_background"):
        assert callable(getattr(volren_amd.Renderer, name)) and "resolve" in getattr(volren_amd.Renderer, name).__doc__
    prop = volren_amd.ShardedRenderer.denoise_resolve
    assert isinstance(prop, property) and prop.fset is not None and "part 0" in prop.__doc__
    assert callable(volpy.Renderer.resolve) and callable(volpy.Renderer.resolved_data) and "fbo_data()'s shape" in volpy.Renderer.resolved_data.__doc__
    assert "denoise_resolve" in volpy._PASS_THROUGH                         # read and written through volpy.Renderer


def test_the_cli_takes_resolve_only_with_two_or_more_expected_rays():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--resolve",), "--resolve needs --expected-features N with N >= 2"),
                         (("--denoise", "--resolve"), "--resolve needs --expected-features N with N >= 2"),
                         (("--resolve", "--expected-features", "1"), "one ray gives the coverage of the pixel's centre"),
                         (("--denoise-temporal", "--resolve", "--expected-features", "1"), "--resolve needs --expected-features N with N >= 2"),
                         (("--resolve", "--expected-features", "2", "--gpus", "2"), "--resolve renders on one device only")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
