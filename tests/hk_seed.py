"""ctypes binding of tests/hostkernel/libseed_host.so: the path-seed table's index (vr_tiles.h) and fill expression (vr_trace.h) built for the host.
TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
from hk_common import _p

_lib = None


def build():
    return hk_common.build(__file__, "seed_host.cpp", "libseed_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_seed_path.restype = C.c_uint32
        L.hk_seed_path.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int]
        L.hk_seed_sub_of_pixel.restype = C.c_uint32
        L.hk_seed_fill.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def index(s, n_frame_tiles, tile, sub, lane):
    """seed_table_index over broadcast arguments: (size_t results as uint64, uint32_t results)"""
    args = np.broadcast_arrays(s, tile, sub, lane)
    a = [np.ascontiguousarray(x, np.uint32).reshape(-1) for x in args]
    o64 = np.zeros(a[0].size, np.uint64)
    o32 = np.zeros(a[0].size, np.uint32)
    lib().hk_seed_index(int(a[0].size), _p(a[0]), int(n_frame_tiles), _p(a[1]), _p(a[2]), _p(a[3]), _p(o64), _p(o32))
    return o64.reshape(args[0].shape), o32.reshape(args[0].shape)


def fill(seed, w, h, a, b):
    """the table entries of the 0-based sample numbers [a, b) of a w x h frame, as seed_fill_kernel lays them out (entry 0 = sample a)"""
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    out = np.zeros((b - a) * n_tiles * 256, np.uint32)
    lib().hk_seed_fill(int(seed) & 0xFFFFFFFF, int(w), int(h), int(a), int(b), _p(out))
    return out


def path_seed(seed, w, px, py, smp):
    return int(lib().hk_seed_path(int(seed) & 0xFFFFFFFF, int(w), int(px), int(py), int(smp)))


def sub_of_pixel(px, py):
    return int(lib().hk_seed_sub_of_pixel(int(px), int(py)))
