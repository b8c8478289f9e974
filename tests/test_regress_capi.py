"""CPU: the public surface of the one-pass regression -- the settings "denoise_filter" and "denoise_ridge" stated in every layer's table and documented, taken
and range-checked (where a renderer can exist; tests/test_gpu_regress.py runs the same checks, every refusal of the calls and the dropped history on the
device); the Python, volpy and command-line layers above them.  What the filter computes: tests/test_regress_host.py on the host build,
tests/test_gpu_regress.py on the device."""
import ctypes as C
import os
import subprocess

import numpy as np

import hk_regress as hg
import scenes
import volren_amd

VR_OK, VR_ERR = 0, 1


def test_the_settings_are_rows_of_every_table_and_documented():
    import volren_amd.volpy as volpy
    from volren_amd import renderer
    capi = open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "capi.cpp")).read()
    assert '{ "denoise_filter", ' in capi and 'if (n == "denoise_ridge")' in capi
    assert "denoise_filter" in renderer._INT_FIELDS and renderer._FLOAT_FIELDS["denoise_ridge"] == 1
    assert "denoise_filter" in volpy._PASS_THROUGH and "denoise_ridge" in volpy._PASS_THROUGH
    for name in ("denoise_filter", "denoise_ridge"):
        prop = getattr(volren_amd.ShardedRenderer, name)
        assert isinstance(prop, property) and prop.fset is not None and "part 0" in prop.__doc__
    assert "denoise_filter" in volren_amd.Renderer.denoise.__doc__ and "denoise_ridge" in volren_amd.Renderer.denoise.__doc__
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    at = text.index("The filter of the layer:")
    doc = text[at:text.index("*/", at)]
    for words in ('"denoise_filter"', '"denoise_ridge"', "default 0", "drops the history", '"denoise_layers" = 1', "11 x 11", "2^-20", "bit for bit", "vr_regress.h", "VR_ERR",
                  "zero order", '"denoise_iterations" = 0'):
        assert words in doc, words
    header = open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_regress.h")).read()
    for words in ("F_p.rgb = kappa_p * Ct", "comes out as B bit for bit", "A_00 <= 2^-20", "dy = -5..5 outer", "rl = lambda * A_00"):
        assert words in header, words
    for doc in ("README.md", "DESIGN.md"):
        body = open(os.path.join(scenes.ROOT, doc)).read()
        assert "denoise_filter" in body and "denoise_ridge" in body and "vr_regress.h" in body, doc


def check_settings(r):
    """"denoise_filter" and "denoise_ridge" on renderer r: the defaults, the values taken, the values refused (which keep the old one)"""
    lib = volren_amd.load()
    assert r.get_int("denoise_filter") == 0 and r.denoise_ridge == hg.default_ridge()
    for v in (1, 0):
        r.denoise_filter = v
        assert r.get_int("denoise_filter") == v and r.denoise_filter == v
        for bad in (-1, 2, 2 ** 31 - 1):
            assert lib.vr_set_int(r._h, b"denoise_filter", bad) == VR_ERR and b"denoise_filter" in lib.vr_last_error(), bad
            assert r.get_int("denoise_filter") == v
    for v in (2.0 ** -20, 1.0, 2.0 ** 20, 0.0, 0.01):
        r.denoise_ridge = v
        assert r.denoise_ridge == np.float32(v)
        for bad in (2.0 ** -21, -1.0, 2.0 ** 20 * 1.5, float("nan"), float("inf")):
            value = (C.c_float * 1)(bad)
            assert lib.vr_set_float(r._h, b"denoise_ridge", value, 1) == VR_ERR and b"denoise_ridge" in lib.vr_last_error(), bad
            assert r.denoise_ridge == np.float32(v)
    two = (C.c_float * 2)(1.0, 1.0)
    assert lib.vr_set_float(r._h, b"denoise_ridge", two, 2) != VR_OK
    r.denoise_ridge = hg.default_ridge()


def test_the_settings_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        r = volren_amd.Renderer(16, 16)
        check_settings(r)
        r.close()


def test_the_cli_takes_the_flags_only_with_the_layered_filter():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--denoise-filter", "1"), "--denoise-filter needs --denoise-layers"),
                         (("--denoise", "--expected-features", "2", "--denoise-filter", "1"), "--denoise-filter needs --denoise-layers"),
                         (("--denoise", "--expected-features", "2", "--denoise-ridge", "0.5"), "--denoise-ridge needs --denoise-layers"),
                         (("--denoise", "--denoise-layers", "--expected-features", "2", "--denoise-filter", "2"), "--denoise-filter: 0 (the a-trous iterations) or 1"),
                         (("--denoise", "--denoise-layers", "--expected-features", "2", "--denoise-filter"), "missing value after --denoise-filter"),
                         (("--denoise", "--denoise-layers", "--expected-features", "2", "--denoise-ridge", "1e-9"), "--denoise-ridge: the ridge must be 0 (zero order) or in [2^-20, 2^20]"),
                         (("--denoise", "--denoise-layers", "--expected-features", "2", "--denoise-ridge", "-1"), "--denoise-ridge: the ridge must be 0 (zero order) or in [2^-20, 2^20]"),
                         (("--denoise-layers", "--denoise-filter", "1"), "--denoise-layers needs --denoise or --denoise-temporal")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
