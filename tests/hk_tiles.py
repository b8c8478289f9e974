"""ctypes binding of tests/hostkernel/libtiles_host.so: the product's tile layout (vr_tiles.h) built for the host.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
from hk_common import _p

_lib = None


def build():
    return hk_common.build(__file__, "tiles_host.cpp", "libtiles_host.so", ("-Wno-unknown-pragmas",))


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_tiles_of_pixel.restype = C.c_int
        L.hk_tiles_variance_scale.restype = C.c_float
        L.hk_tiles_variance_scale.argtypes = [C.c_int]
        _lib = L
    return _lib


def grid(w, h):
    """(tiles_x, tiles_y, tile count)"""
    out = np.zeros(3, np.int32)
    lib().hk_tiles_grid(int(w), int(h), _p(out))
    return tuple(int(v) for v in out)


def tile_of_pixel(px, py, w):
    return int(lib().hk_tiles_of_pixel(int(px), int(py), int(w)))


def pixels(tile, w, raster=False):
    """[256][5] = (tile, sub, lane, px, py) of every thread of the workgroup that serves `tile`"""
    out = np.zeros((256, 5), np.int32)
    lib().hk_tiles_pixels(1 if raster else 0, int(tile), int(w), _p(out))
    return out


def pool_slots(chunk, n_tiles, tile_slot, sub, spu, sample, lane):
    """pool_slot over broadcast arguments: (size_t results as uint64, uint32_t results)"""
    args = np.broadcast_arrays(chunk, tile_slot, sub, sample, lane)
    a = [np.ascontiguousarray(x, np.uint32).reshape(-1) for x in args]
    o64 = np.zeros(a[0].size, np.uint64)
    o32 = np.zeros(a[0].size, np.uint32)
    lib().hk_tiles_pool_slots(int(a[0].size), _p(a[0]), int(n_tiles), _p(a[1]), _p(a[2]), int(spu), _p(a[3]), _p(a[4]), _p(o64), _p(o32))
    return o64.reshape(args[0].shape), o32.reshape(args[0].shape)


def window(r, tile, w):
    """TileWindow<r> of `tile`: (kFoot, kTexels, x0, y0) and at[256], the window index of every wave-tiled thread's pixel"""
    geom = np.zeros(4, np.int32)
    at = np.zeros(256, np.int32)
    assert lib().hk_tiles_window(int(r), int(tile), int(w), _p(geom), _p(at)) == 0, r
    return tuple(int(v) for v in geom), at


def variance_scale(n):
    return np.float32(lib().hk_tiles_variance_scale(int(n)))
