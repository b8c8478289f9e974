"""CPU: the C ABI of adaptive sampling (vr_render_adaptive, vr_tile_samples, vr_tile_error) -- exported, listed, documented, and failing loudly
without a device or a renderer."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NEW = ("vr_render_adaptive", "vr_tile_samples", "vr_tile_error")


def test_new_symbols_are_exported_and_listed():
    lib = volren_amd.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in volren_amd.SYMBOLS, n
        assert n in declared_functions(), n
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    assert "ragged" in text.lower() and "min_spp at 16" in text and "biased" in text


def test_null_renderer_is_rejected():
    lib = volren_amd.load()
    ibuf = np.zeros(64, np.int32)
    fbuf = np.zeros(64, np.float32)
    assert lib.vr_render_adaptive(None, 4, 64, 0.1) == 3 and b"null renderer" in lib.vr_last_error()      # VR_ERR_ARG
    assert lib.vr_tile_samples(None, ibuf.ctypes.data, 1) == 3
    assert lib.vr_tile_error(None, fbuf.ctypes.data, 1) == 3


def test_bad_arguments_are_rejected_before_the_device():
    lib = volren_amd.load()
    fake = C.create_string_buffer(256)                      # never dereferenced: the arguments are checked first
    for mn, mx, t in ((1, 64, 0.1), (0, 64, 0.1), (65, 64, 0.1), (4, 64, -0.5), (4, 64, float("nan")), (4, 64, float("inf"))):
        assert lib.vr_render_adaptive(C.addressof(fake), mn, mx, t) == 3, (mn, mx, t)
    assert lib.vr_tile_samples(C.addressof(fake), None, 1) == 3
    assert lib.vr_tile_error(C.addressof(fake), None, 1) == 3


def test_new_entry_points_need_a_device():
    lib = volren_amd.load()
    if lib.vr_device_count() > 0:
        pytest.skip("a HIP device is present")
    fake = C.create_string_buffer(256)                      # never dereferenced: the device check comes first
    ibuf = np.zeros(64, np.int32)
    fbuf = np.zeros(64, np.float32)
    assert lib.vr_render_adaptive(C.addressof(fake), 16, 1024, 0.05) == 2          # VR_ERR_NO_DEVICE
    assert b"no HIP device" in lib.vr_last_error()
    assert lib.vr_render_adaptive(C.addressof(fake), 2, 2, 0.0) == 2
    assert lib.vr_tile_samples(C.addressof(fake), ibuf.ctypes.data, 1) == 2
    assert lib.vr_tile_error(C.addressof(fake), fbuf.ctypes.data, 1) == 2
