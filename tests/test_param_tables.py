"""CPU: the tables that state the named parameters and the exported symbols, one per layer, agree with each other -- renderer.py's name lists against
capi.cpp's rows (read as text: no renderer exists without a device), volpy's pass-through names against renderer.py's, _lib.py's signatures against the
header.  tests/test_gpu_params.py reads and writes every name on a live renderer."""
import os
import re

import scenes
import volren_amd.volpy as volpy
from test_capi_symbols import declared_functions
from volren_amd import _lib, renderer

CAPI = open(os.path.join(scenes.ROOT, "volren_amd", "csrc", "capi.cpp")).read()


def _between(text, start, end):
    at = text.index(start)
    return text[at:text.index(end, at)]


def int_rows():
    """name -> the text of its row in capi.cpp's kIntParams"""
    body = _between(CAPI, "const IntParam kIntParams[] = {", "\n};")
    return {m.group(1): m.group(0) for m in re.finditer(r'^    \{ "(\w+)",.*$', body, flags=re.M)}


def float_rows():
    return set(re.findall(r'if \(n == "(\w+)"\)', _between(CAPI, "FloatField float_field(", "unknown float parameter")))


def test_every_python_int_name_is_a_row_of_the_c_table_and_as_writable_as_python_says():
    rows = int_rows()
    assert len(rows) >= 40 and len(rows) == CAPI.count('\n    { "')          # every row was read, none twice
    for name in renderer._INT_FIELDS:
        assert name in rows and "VR_READ_ONLY" not in rows[name], name
    for name in renderer._READ_ONLY_INT_FIELDS:
        assert name in rows and "VR_READ_ONLY" in rows[name], name
    # the rows Python does not list: the frame's size, which the Python object keeps itself
    assert set(rows) - set(renderer._INT_FIELDS) - set(renderer._READ_ONLY_INT_FIELDS) == {"width", "height"}


def test_no_int_name_is_both_settable_and_read_only():
    both = set(renderer._INT_FIELDS) & set(renderer._READ_ONLY_INT_FIELDS)
    assert not both, both
    for names in (renderer._INT_FIELDS, renderer._READ_ONLY_INT_FIELDS):
        assert len(set(names)) == len(names)


def test_every_python_float_name_is_a_row_of_the_c_table():
    assert float_rows() == set(renderer._FLOAT_FIELDS)


def test_the_names_volpy_passes_through_are_names_the_renderer_knows():
    known = set(renderer._INT_FIELDS) | set(renderer._FLOAT_FIELDS)
    assert volpy._PASS_THROUGH and not set(volpy._PASS_THROUGH) - known
    assert not set(volpy._PASS_THROUGH) & (set(volpy._SCALARS) | set(volpy._VEC3S))
    assert not (set(volpy._SCALARS) | set(volpy._VEC3S)) - known


def test_the_signature_table_is_the_header():
    assert sorted(_lib._SIGNATURES) == declared_functions() and _lib.SYMBOLS == list(_lib._SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in _lib._SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype == restype, name
