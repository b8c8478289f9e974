"""CPU: the C ABI of the denoiser data (vr_render_features, vr_features, vr_variance, vr_set_int "variance") -- exported, listed, documented,
and failing loudly without a device or a renderer."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NEW = ("vr_render_features", "vr_features", "vr_variance")


def test_new_symbols_are_exported_and_listed():
    lib = volren_amd.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in volren_amd.SYMBOLS, n
        assert n in declared_functions(), n
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    assert '"variance"' in text


def test_variance_round_trips_through_set_and_get_int():
    lib = volren_amd.load()
    if lib.vr_device_count() <= 0:
        pytest.skip("needs a HIP device (a renderer)")
    r = volren_amd.Renderer(16, 16)
    assert r.get_int("variance") == 0
    r.variance = 1
    assert r.get_int("variance") == 1
    v = C.c_int()
    assert lib.vr_get_int(r._h, b"variance", C.byref(v)) == 0 and v.value == 1
    assert lib.vr_set_int(r._h, b"variance", 2) == 1                # VR_ERR: 0 or 1
    r.variance = 0
    assert r.get_int("variance") == 0


def test_new_entry_points_need_a_device():
    lib = volren_amd.load()
    if lib.vr_device_count() > 0:
        pytest.skip("a HIP device is present")
    fake = C.create_string_buffer(256)                              # never dereferenced: the device check comes first
    buf = np.zeros(64, np.float32)
    assert lib.vr_render_features(C.addressof(fake), 4) == 2        # VR_ERR_NO_DEVICE
    assert b"no HIP device" in lib.vr_last_error()
    assert lib.vr_features(C.addressof(fake), buf.ctypes.data) == 2
    assert lib.vr_variance(C.addressof(fake), buf.ctypes.data) == 2


def test_null_renderer_is_rejected():
    lib = volren_amd.load()
    buf = np.zeros(64, np.float32)
    assert lib.vr_render_features(None, 4) == 3 and b"null renderer" in lib.vr_last_error()      # VR_ERR_ARG
    assert lib.vr_features(None, buf.ctypes.data) == 3
    assert lib.vr_variance(None, buf.ctypes.data) == 3
