"""CPU: the C ABI of the temporal luminance moments (vr_set_int / vr_get_int "denoise_moments", vr_denoise_history_moments) -- exported, listed,
documented with its range, what a change does and the refusal with rejection, and failing loudly without a renderer, an output or a device.  The
check of the values needs a renderer, which needs a device: where one is present it runs here too, and tests/test_gpu_moments.py runs it in any case."""
import ctypes as C
import os

import numpy as np

import scenes
import volren_amd
from test_capi_symbols import declared_functions

INT_MAX = 2 ** 31 - 1


def test_the_new_symbol_is_exported_listed_and_documented():
    lib = volren_amd.load()
    assert hasattr(lib, "vr_denoise_history_moments")
    assert "vr_denoise_history_moments" in volren_amd.SYMBOLS and "vr_denoise_history_moments" in declared_functions()
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    assert '"denoise_moments"' in text and "drops the history" in text and "vr_moments.h" in text
    at = text.index('"denoise_moments" = 1 and "denoise_reject" > 0')       # the refusal names both settings
    assert "VR_ERR" in text[at:at + 200]
    assert os.path.exists(os.path.join(scenes.ROOT, "volren_amd", "csrc", "vr_moments.h"))


def test_refusals_of_the_moment_records():
    lib = volren_amd.load()
    buf = np.zeros(64, np.float32)
    assert lib.vr_denoise_history_moments(None, buf.ctypes.data) == 3 and b"null renderer" in lib.vr_last_error()      # VR_ERR_ARG
    fake = C.create_string_buffer(256)                              # never dereferenced: the argument and device checks come first
    assert lib.vr_denoise_history_moments(C.addressof(fake), None) == 3 and b"null argument" in lib.vr_last_error()
    if lib.vr_device_count() <= 0:
        assert lib.vr_denoise_history_moments(C.addressof(fake), buf.ctypes.data) == 2 and b"no HIP device" in lib.vr_last_error()      # VR_ERR_NO_DEVICE


def check_values(r):
    """vr_set_int "denoise_moments" on renderer r: 0 and 1 are taken, -1, 2 and INT_MAX are VR_ERR and keep the old value"""
    lib = volren_amd.load()
    assert r.denoise_moments == 0                                   # off by default
    for v in (1, 0, 1):
        r.denoise_moments = v
        assert r.denoise_moments == v and r.get_int("denoise_moments") == v
        for bad in (-1, 2, INT_MAX):
            assert lib.vr_set_int(r._h, b"denoise_moments", bad) == 1, bad
            assert b"denoise_moments" in lib.vr_last_error()
            assert r.denoise_moments == v


def test_the_values_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        check_values(volren_amd.Renderer(16, 16))


def test_the_python_layers_carry_the_new_names():
    import volren_amd.volpy as volpy
    from volren_amd import renderer
    assert "denoise_moments" in renderer._INT_FIELDS
    assert callable(volren_amd.Renderer.denoise_history_moments) and callable(volren_amd.ShardedRenderer.denoise_history_moments)
    assert isinstance(volren_amd.ShardedRenderer.denoise_moments, property)
    assert callable(volpy.Renderer.denoise_history_moments_data)
    src = open(volpy.__file__).read()
    assert '"denoise_moments"' in src


def test_the_cli_refuses_the_flag_alone_and_with_rejection():
    """both refusals come before the first device call"""
    import subprocess
    exe = os.path.join(scenes.ROOT, "volren_amd", "volren")
    for flags, words in ((("--denoise-moments",), "--denoise-moments needs --denoise-temporal"),
                         (("--denoise", "--denoise-moments"), "--denoise-moments needs --denoise-temporal"),
                         (("--denoise-temporal", "--denoise-moments", "--denoise-reject", "3"), "--denoise-moments and --denoise-reject")):
        out = subprocess.run([exe, "-w", "16", "-h", "16", "--render"] + list(flags), capture_output=True, text=True, timeout=60)
        assert out.returncode != 0 and words in out.stderr, (flags, out.stderr[-500:])
