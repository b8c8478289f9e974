"""CPU: the public surface of "denoise_demodulate" -- the row of capi.cpp's table, the Python, volpy and command-line layers above it, the documentation,
the refusals stated where they are made (check_setting below holds the setting's range and runs from tests/test_gpu_demod.py, which also has every refusal
of the calls and the dropped history on the device).  What the setting computes: tests/test_demod_host.py on the host build, tests/test_gpu_demod.py on the device."""
import os
import subprocess

import scenes
import volren_amd
import volren_amd.volpy as volpy
from test_param_tables import int_rows
from volren_amd import renderer

VR_ERR = 1


def _text(*path):
    return open(os.path.join(scenes.ROOT, *path)).read()


def test_the_setting_is_a_row_of_the_c_table_and_a_name_of_every_python_layer():
    row = int_rows()["denoise_demodulate"]
    assert "R.set_denoise_demodulate(v)" in row and "VR_READ_ONLY" not in row
    assert "denoise_demodulate" in renderer._INT_FIELDS and "denoise_demodulate" in volpy._PASS_THROUGH
    prop = volren_amd.ShardedRenderer.denoise_demodulate
    assert isinstance(prop, property) and prop.fset is not None and "part 0" in prop.__doc__
    assert "denoise_demodulate" in volren_amd.Renderer.denoise.__doc__ and "denoise_demodulate" in volpy.Renderer.denoised_layer_data.__doc__


def test_the_calls_refuse_before_anything_is_launched():
    """read from the source, in order: run_denoise states the refusal of 1 without denoise_layers = 1 before its first allocation and launch, the sharded
    renderer before its exchange (tests/test_gpu_demod.py has the behaviour on the device)"""
    src = _text("volren_amd", "csrc", "renderer.cpp")
    body = src[src.index("void RendererHIP::run_denoise("):src.index("void RendererHIP::drop_history()")]
    at = body.index("denoise_demodulate = 1 needs denoise_layers = 1")
    assert at < body.index("ensure_buffer(") and at < body.index("launch_") and at < body.index("run_resolve()")
    sharded = _text("volren_amd", "csrc", "sharded.cpp")
    body = sharded[sharded.index("void ShardedRenderer::run_denoise("):sharded.index("void ShardedRenderer::denoise()")]
    assert body.index("denoise_demodulate = 1 needs denoise_layers = 1") < body.index("exchange_guides();")


def test_the_documents_state_it():
    header = _text("include", "volren_amd.h")
    at = header.index("Albedo demodulation:")
    doc = header[at:header.index("*/", at)]
    for words in ('"denoise_demodulate"', "default 0", "drops the history", '"denoise_layers" = 1', "2^-6", "bit for bit", "vr_demod.h", "VR_ERR", "vr_upsample", "emission"):
        assert words in doc, words
    lane = _text("volren_amd", "csrc", "vr_demod.h")
    for words in ("kDemodFloor = 2^-6", "S_p.rgb = (y_p.rgb - G_p) / d", "t_c = sqrt_(max_(var_c, 0)) / d_c", "L.rgb = L.rgb * d", "What the floor costs", "kappa_p = 0: d = 1"):
        assert words in lane, words
    for path in (("INTEGRATION.md",), ("DESIGN.md",), ("README.md",)):
        assert "denoise_demodulate" in _text(*path), path
    assert "--denoise-demodulate" in _text("README.md")


def check_setting(r):
    """"denoise_demodulate" on renderer r: the default, the values taken, the values refused (which keep the old one)"""
    lib = volren_amd.load()
    assert r.get_int("denoise_demodulate") == 0 and r.denoise_demodulate == 0
    for v in (1, 0):
        r.denoise_demodulate = v
        assert r.get_int("denoise_demodulate") == v and r.denoise_demodulate == v
        for bad in (-1, 2, 2 ** 31 - 1):
            assert lib.vr_set_int(r._h, b"denoise_demodulate", bad) == VR_ERR and b"denoise_demodulate" in lib.vr_last_error(), bad
            assert r.get_int("denoise_demodulate") == v


def test_the_cli_takes_the_flag_only_with_the_layered_filter():
    """the refusals come before the first device call"""
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--denoise-demodulate",), "--denoise-demodulate needs --denoise-layers"),
                         (("--denoise", "--expected-features", "2", "--denoise-demodulate"), "--denoise-demodulate needs --denoise-layers"),
                         (("--denoise-temporal", "--expected-features", "2", "--upsample", "2", "--denoise-demodulate"), "--denoise-demodulate needs --denoise-layers"),
                         (("--denoise-layers", "--denoise-demodulate"), "--denoise-layers needs --denoise or --denoise-temporal")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
