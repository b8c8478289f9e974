"""CPU: the public surface of "expected_field" -- the row of capi.cpp's table, the Python, volpy and command-line layers above it, the documentation.
What the setting computes: tests/test_expected_cubic_host.py on the host build, tests/test_gpu_expected_cubic.py on the device."""
import os
import subprocess

import scenes
import volren_amd
import volren_amd.volpy as volpy
from test_param_tables import int_rows
from volren_amd import renderer


def test_the_setting_is_a_row_of_the_c_table_and_a_name_of_every_python_layer():
    row = int_rows()["expected_field"]
    assert "VR_INT(expected_field), 0, 1," in row and "set_history_switch" not in row       # a plain field: changing it drops no temporal history
    assert "expected_field" in renderer._INT_FIELDS and "expected_field" in volpy._PASS_THROUGH
    prop = volren_amd.ShardedRenderer.expected_field
    assert isinstance(prop, property) and prop.fset is not None and "every part" in prop.__doc__
    assert "expected_field" in volpy.Renderer.render_features_expected.__doc__ and "expected_field" in volren_amd.Renderer.render_features_expected.__doc__
    assert len(volren_amd.Renderer.PROBE_OUT_WORDS) == 9 and volren_amd.Renderer.PROBE_OUT_WORDS[8] == 4


def test_the_documents_state_it():
    def text(*path):
        return open(os.path.join(scenes.ROOT, *path)).read()
    header = text("include", "volren_amd.h")
    at = header.index('vr_set_int "expected_field"')
    doc = header[at:at + 2500]
    for words in ("the default", "cubic B-spline", "transfer function", "reach 2", "vr_cubic.h", "history"):
        assert words in doc, words
    for path in (("INTEGRATION.md",), ("DESIGN.md",), ("README.md",)):
        assert "expected_field" in text(*path), path
    assert "CUBIC" in text("volren_amd", "csrc", "vr_expected.h") and "reach 2" in text("volren_amd", "csrc", "vr_clear.h")


def test_the_cli_takes_the_flag_only_with_expected_features_and_only_0_or_1():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--denoise", "--expected-field", "1"), "--expected-field needs --expected-features"),
                         (("--expected-field", "0"), "--expected-field needs --expected-features"),
                         (("--denoise", "--expected-features", "2", "--expected-field", "2"), "--expected-field: 0 (the trilinear field) or 1"),
                         (("--denoise", "--expected-features", "2", "--expected-field", "-1"), "--expected-field: 0 (the trilinear field) or 1"),
                         (("--denoise", "--expected-features", "2", "--expected-field"), "missing value after --expected-field")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
