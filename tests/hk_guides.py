"""ctypes binding of tests/hostkernel/libguides_host.so: the wire format of the sharded renderer's packed denoiser guides (vr_tiles.h guide_slot)
built for the host.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common

_lib = None


def build():
    return hk_common.build(__file__, "guides_host.cpp", "libguides_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_guides_planes.restype = C.c_int
        L.hk_guides_slots.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
        L.hk_guides_pixels.argtypes = [C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def planes():
    return int(lib().hk_guides_planes())


def slots(first, n):
    """[n][planes][256] uint64: the float4 index of (tile slot first + k, plane, thread)"""
    out = np.zeros((int(n), planes(), 256), np.uint64)
    lib().hk_guides_slots(int(first), int(n), out.ctypes.data_as(C.c_void_p))
    return out


def pixels(tile, w):
    """[256][2] int32 = (px, py) of every thread of the workgroup that serves `tile` (raster in the tile)"""
    out = np.zeros((256, 2), np.int32)
    lib().hk_guides_pixels(int(tile), int(w), out.ctypes.data_as(C.c_void_p))
    return out
