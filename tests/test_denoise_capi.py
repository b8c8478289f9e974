"""CPU: the C ABI of the denoiser (vr_denoise, vr_denoised, vr_set_int "denoise_iterations", vr_set_float "denoise_sigma") -- exported, listed,
documented, and failing loudly without a device or a renderer."""
import ctypes as C
import os

import numpy as np
import pytest

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NEW = ("vr_denoise", "vr_denoised")


def test_new_symbols_are_exported_and_listed():
    lib = volren_amd.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in volren_amd.SYMBOLS, n
        assert n in declared_functions(), n
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    assert '"denoise_iterations"' in text and '"denoise_sigma"' in text and "datagen_denoise.py" in text


def test_null_renderer_is_rejected():
    lib = volren_amd.load()
    buf = np.zeros(64, np.float32)
    assert lib.vr_denoise(None) == 3 and b"null renderer" in lib.vr_last_error()      # VR_ERR_ARG
    assert lib.vr_denoised(None, buf.ctypes.data) == 3


def test_new_entry_points_need_a_device():
    lib = volren_amd.load()
    if lib.vr_device_count() > 0:
        pytest.skip("a HIP device is present")
    fake = C.create_string_buffer(256)                              # never dereferenced: the device check comes first
    buf = np.zeros(64, np.float32)
    assert lib.vr_denoise(C.addressof(fake)) == 2                   # VR_ERR_NO_DEVICE
    assert b"no HIP device" in lib.vr_last_error()
    assert lib.vr_denoised(C.addressof(fake), buf.ctypes.data) == 2


def test_denoise_settings_range_checks():
    lib = volren_amd.load()
    if lib.vr_device_count() <= 0:
        pytest.skip("needs a HIP device (a renderer)")
    r = volren_amd.Renderer(16, 16)
    assert r.denoise_iterations == 5
    assert np.array_equal(r.denoise_sigma, np.array([4.0, 0.5, 0.1, 0.25, 0.2], np.float32))
    for v in (0, 3, 10):
        r.denoise_iterations = v
        assert r.denoise_iterations == v
    for v in (-1, 11):
        assert lib.vr_set_int(r._h, b"denoise_iterations", v) == 1 and b"denoise_iterations" in lib.vr_last_error()
    assert r.denoise_iterations == 10
    r.denoise_sigma = (1, 2, 3, 4, 5)
    assert np.array_equal(r.denoise_sigma, np.arange(1, 6, dtype=np.float32))
    for bad in ((1, 2, 3, 4, 0), (1, -2, 3, 4, 5), (np.inf, 2, 3, 4, 5), (1, 2, np.nan, 4, 5)):
        v = np.asarray(bad, np.float32)
        assert lib.vr_set_float(r._h, b"denoise_sigma", v.ctypes.data_as(C.POINTER(C.c_float)), 5) == 1
    v = np.ones(4, np.float32)
    assert lib.vr_set_float(r._h, b"denoise_sigma", v.ctypes.data_as(C.POINTER(C.c_float)), 4) == 1
    assert np.array_equal(r.denoise_sigma, np.arange(1, 6, dtype=np.float32))       # refused values leave the old ones
    # [2^-60, 2^60]: sigma_a^2 stays a normal float (sigma_a = 1e-23 gave 0 / 0 = NaN for equal albedos); the ends themselves are accepted
    lo, hi = np.float32(2.0 ** -60), np.float32(2.0 ** 60)
    for i in range(5):
        for bad in (np.nextafter(lo, np.float32(0)), np.float32(1e-23), np.float32(2.0 ** -100), np.nextafter(hi, np.float32(np.inf)), np.float32(1e30)):
            v = np.arange(1, 6, dtype=np.float32)
            v[i] = bad
            assert lib.vr_set_float(r._h, b"denoise_sigma", v.ctypes.data_as(C.POINTER(C.c_float)), 5) == 1, (i, bad)
            assert b"2^-60" in lib.vr_last_error()
            assert np.array_equal(r.denoise_sigma, np.arange(1, 6, dtype=np.float32))
    for v in ((lo,) * 5, (hi,) * 5, (lo, hi, lo, hi, lo)):
        r.denoise_sigma = v
        assert np.array_equal(r.denoise_sigma, np.asarray(v, np.float32))
