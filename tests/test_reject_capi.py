"""CPU: the C ABI of the history rejection (vr_set_float / vr_get_float "denoise_reject", vr_denoise_reject_stat) -- exported, listed, documented with
its range and its two limits, and failing loudly without a renderer, an output or a device.  The range check needs a renderer, which needs a
device: where one is present it runs here too, and tests/test_gpu_reject.py runs it in any case."""
import ctypes as C
import os

import numpy as np

import scenes
import volren_amd
from test_capi_symbols import declared_functions


def test_the_new_symbol_is_exported_listed_and_documented():
    lib = volren_amd.load()
    assert hasattr(lib, "vr_denoise_reject_stat")
    assert "vr_denoise_reject_stat" in volren_amd.SYMBOLS and "vr_denoise_reject_stat" in declared_functions()
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    assert '"denoise_reject"' in text and "[2^-10, 2^20]" in text and "0 = off" in text
    assert "n >= 2 samples per pixel" in text and "far above 1e-6" in text      # the two limits


def test_refusals_of_the_statistic():
    lib = volren_amd.load()
    buf = np.zeros(64, np.float32)
    assert lib.vr_denoise_reject_stat(None, buf.ctypes.data) == 3 and b"null renderer" in lib.vr_last_error()      # VR_ERR_ARG
    fake = C.create_string_buffer(256)                              # never dereferenced: the argument and device checks come first
    assert lib.vr_denoise_reject_stat(C.addressof(fake), None) == 3 and b"null argument" in lib.vr_last_error()
    if lib.vr_device_count() <= 0:
        assert lib.vr_denoise_reject_stat(C.addressof(fake), buf.ctypes.data) == 2 and b"no HIP device" in lib.vr_last_error()      # VR_ERR_NO_DEVICE


def check_range(r):
    """vr_set_float "denoise_reject" on renderer r: 0 and [2^-10, 2^20] are taken, everything else is VR_ERR and keeps the old value"""
    lib = volren_amd.load()
    assert r.denoise_reject == 0.0                                  # off by default
    for v in (2.0 ** -10, 3.0, 2.0 ** 20, 0.0, 0.5):
        r.denoise_reject = v
        assert r.denoise_reject == np.float32(v)
    lo, hi = np.float32(2.0 ** -10), np.float32(2.0 ** 20)
    for bad in (-0.5, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf)), np.float32(1e-30), np.inf, -np.inf, np.nan):
        v = np.asarray([bad], np.float32)
        assert lib.vr_set_float(r._h, b"denoise_reject", v.ctypes.data_as(C.POINTER(C.c_float)), 1) == 1, bad
        assert b"denoise_reject" in lib.vr_last_error() and b"2^-10" in lib.vr_last_error()
        assert r.denoise_reject == 0.5
    v = np.asarray([3.0, 3.0], np.float32)
    assert lib.vr_set_float(r._h, b"denoise_reject", v.ctypes.data_as(C.POINTER(C.c_float)), 2) == 1
    assert r.denoise_reject == 0.5


def test_the_range_of_the_threshold_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        check_range(volren_amd.Renderer(16, 16))


def test_the_python_layers_carry_the_new_names():
    import volren_amd.volpy as volpy
    from volren_amd import renderer
    assert renderer._FLOAT_FIELDS["denoise_reject"] == 1
    assert callable(volren_amd.Renderer.denoise_reject_stat) and callable(volren_amd.ShardedRenderer.denoise_reject_stat)
    assert isinstance(volren_amd.ShardedRenderer.denoise_reject, property)
    assert callable(volpy.Renderer.denoise_reject_stat_data)
