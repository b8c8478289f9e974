"""GPU: every named parameter of renderer.py's lists on one live 16x16 renderer (config c3: a volume, an environment and a transfer function, so every
name has something behind it) -- read, written back with its own value, refused where it is read-only, has the wrong count or is out of range, with the
refusal's own words and the value left as it was.  No sample is rendered.  A name that Python lists and the library's tables (capi.cpp) do not know, or
know otherwise, fails here; tests/test_param_tables.py compares the lists as text without a device."""
import ctypes as C

import numpy as np
import pytest

import scenes
import volren_amd
from volren_amd import renderer

pytestmark = pytest.mark.gpu

VR_OK, VR_ERR = 0, 1
# one value outside the accepted range of every int row that has one (or whose writer refuses by itself), with words of that row's refusal
INT_REFUSALS = (("variance", 2, "variance: 0 (off) or 1"), ("denoise_iterations", 11, "denoise_iterations must be in [0, 10]"),
                ("denoise_moments", 2, "denoise_moments: 0 (the frames' sample variance) or 1"), ("denoise_resolve", 2, "denoise_resolve: 0 (the filter starts from the framebuffer) or 1"),
                ("denoise_layers", -1, "denoise_layers: 0 (the filter runs on the frame) or 1"), ("majorant_layout", -2, "majorant_layout: -1 (per grid, chosen at commit), 0 (linear), 1"),
                ("wide_addressing", 2, "wide_addressing: 0 (by the tables' sizes), 1"), ("sample_pool_mb", 15, "sample_pool_mb must be in [16, 65536]"),
                ("seed_table_mb", 8193, "seed_table_mb must be in [0, 8192]"), ("seed_table_max_samples", -1, "seed_table_max_samples must be >= 0"),
                ("launch_target_ms", -1, "launch_target_ms must be >= 0"), ("expected_skip", 2, "expected_skip: 0 (march every step) or 1"),
                ("expected_stats", -1, "expected_stats: 0 (off) or 1"), ("order_tiles", 3, "order_tiles: 0 (never), 1 (tile subsets), 2 (always)"),
                ("grid_frame_counter", 1, "grid_frame_counter out of range"))          # the scene has one grid frame
FLOAT_REFUSALS = (("denoise_sigma", (1.0, 1.0, 2.0 ** 61, 1.0, 1.0), "denoise_sigma: every value must be in [2^-60, 2^60]"),
                  ("denoise_alpha", (2.0,), "denoise_alpha must be in [2^-20, 1]"), ("denoise_reject", (2.0 ** -11,), "denoise_reject must be 0 (off) or in [2^-10, 2^20]"))


@pytest.fixture(scope="module")
def r():
    r = scenes.hip_scene("c3", 16, 16)
    yield r
    r.close()


def _error(lib):
    return lib.vr_last_error().decode()


def _floats(r, name):
    return np.atleast_1d(np.asarray(getattr(r, name), np.float32))


def _set_float(r, name, values):
    v = np.ascontiguousarray(values, np.float32)
    return r._L.vr_set_float(r._h, name.encode(), v.ctypes.data_as(C.POINTER(C.c_float)), v.size)


def test_every_settable_int_reads_and_takes_its_own_value_back(r):
    bad = []
    for name in renderer._INT_FIELDS:
        try:
            v = r.get_int(name)
            setattr(r, name, v)
            if r.get_int(name) != v:
                bad.append((name, v, r.get_int(name)))
        except volren_amd.VolrenError as e:
            bad.append((name, str(e)))
    assert not bad, bad


def test_every_read_only_int_reads_and_refuses_a_write_as_an_unknown_name(r):
    lib, bad = r._L, []
    for name in renderer._READ_ONLY_INT_FIELDS + ("width", "height"):
        try:
            v = r.get_int(name)
            if name not in ("width", "height") and getattr(r, name) != v:
                bad.append((name, "attribute differs"))
        except volren_amd.VolrenError as e:
            bad.append((name, str(e)))
            continue
        if lib.vr_set_int(r._h, name.encode(), v) != VR_ERR or _error(lib) != "unknown int parameter: " + name or r.get_int(name) != v:
            bad.append((name, "write", _error(lib)))
    assert not bad, bad
    assert r.get_int("width") == 16 and r.get_int("height") == 16
    assert lib.vr_set_int(r._h, b"no_such_name", 0) == VR_ERR and _error(lib) == "unknown int parameter: no_such_name"
    assert lib.vr_get_int(r._h, b"no_such_name", C.byref(C.c_int())) == VR_ERR and _error(lib) == "unknown int parameter: no_such_name"


def test_every_float_field_reads_with_its_count_and_takes_its_own_values_back(r):
    bad = []
    for name, count in renderer._FLOAT_FIELDS.items():
        try:
            v = _floats(r, name)
            setattr(r, name, v)
            if v.size != count or not np.array_equal(_floats(r, name).view(np.uint32), v.view(np.uint32)):
                bad.append((name, v, _floats(r, name)))
        except volren_amd.VolrenError as e:
            bad.append((name, str(e)))
    assert not bad, bad


def test_every_float_field_refuses_one_value_too_many(r):
    """reading: "wrong value count" for every field; writing: the same, but for denoise_sigma, which states its count in words of its own"""
    lib, bad = r._L, []
    for name, count in renderer._FLOAT_FIELDS.items():
        v = _floats(r, name)
        more = np.concatenate([v, v[-1:]])
        out = (C.c_float * (count + 1))()
        if lib.vr_get_float(r._h, name.encode(), out, count + 1) != VR_ERR or _error(lib) != "wrong value count for " + name:
            bad.append((name, "read", _error(lib)))
        words = "denoise_sigma takes 5 values" if name == "denoise_sigma" else "wrong value count for " + name
        if _set_float(r, name, more) != VR_ERR or words not in _error(lib):
            bad.append((name, "write", _error(lib)))
        if not np.array_equal(_floats(r, name).view(np.uint32), v.view(np.uint32)):
            bad.append((name, "changed"))
    assert not bad, bad


def test_a_value_out_of_range_is_refused_in_the_rows_own_words_and_changes_nothing(r):
    lib, bad = r._L, []
    for name, value, words in INT_REFUSALS:
        v = r.get_int(name)
        if lib.vr_set_int(r._h, name.encode(), value) != VR_ERR or words not in _error(lib) or r.get_int(name) != v:
            bad.append((name, _error(lib), v, r.get_int(name)))
    for name, values, words in FLOAT_REFUSALS:
        v = _floats(r, name)
        if _set_float(r, name, values) != VR_ERR or words not in _error(lib) or not np.array_equal(_floats(r, name).view(np.uint32), v.view(np.uint32)):
            bad.append((name, _error(lib)))
    assert not bad, bad
    ranged = {n for n, _, _ in INT_REFUSALS}
    assert ranged <= set(renderer._INT_FIELDS) and {n for n, _, _ in FLOAT_REFUSALS} <= set(renderer._FLOAT_FIELDS)
