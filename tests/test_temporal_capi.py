"""CPU: the C ABI of the temporal accumulation (vr_denoise_temporal, vr_denoise_history_reset, vr_denoise_history, vr_set_float "denoise_alpha") --
exported, listed, documented, and failing loudly without a device or a renderer."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NEW = ("vr_denoise_temporal", "vr_denoise_history_reset", "vr_denoise_history")


def test_new_symbols_are_exported_and_listed():
    lib = volren_amd.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in volren_amd.SYMBOLS, n
        assert n in declared_functions(), n
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    assert '"denoise_alpha"' in text and "[2^-20, 1]" in text and "vr_temporal.h" in text
    assert "once per frame" in text.lower() and "equal samples per pixel" in text


def test_null_renderer_is_rejected():
    lib = volren_amd.load()
    buf = np.zeros(64, np.float32)
    assert lib.vr_denoise_temporal(None) == 3 and b"null renderer" in lib.vr_last_error()      # VR_ERR_ARG
    assert lib.vr_denoise_history_reset(None) == 3 and b"null renderer" in lib.vr_last_error()
    assert lib.vr_denoise_history(None, buf.ctypes.data, None, None) == 3 and b"null renderer" in lib.vr_last_error()


def test_new_entry_points_need_a_device():
    lib = volren_amd.load()
    if lib.vr_device_count() > 0:
        pytest.skip("a HIP device is present")
    fake = C.create_string_buffer(256)                              # never dereferenced: the device check comes first
    buf = np.zeros(64, np.float32)
    assert lib.vr_denoise_temporal(C.addressof(fake)) == 2          # VR_ERR_NO_DEVICE
    assert b"no HIP device" in lib.vr_last_error()
    assert lib.vr_denoise_history_reset(C.addressof(fake)) == 2 and b"no HIP device" in lib.vr_last_error()
    assert lib.vr_denoise_history(C.addressof(fake), buf.ctypes.data, None, None) == 2 and b"no HIP device" in lib.vr_last_error()


def test_the_python_layers_carry_the_new_names():
    import volren_amd.volpy as volpy
    for n in ("denoise_temporal", "denoise_history", "denoise_history_reset"):
        assert callable(getattr(volren_amd.Renderer, n)), n
    for n in ("denoise_temporal", "denoise_history_reset", "denoised_data"):
        assert callable(getattr(volpy.Renderer, n)), n
    from volren_amd import renderer
    assert renderer._FLOAT_FIELDS["denoise_alpha"] == 1
