"""ctypes binding of tests/hostkernel/libhotpair_host*.so: collide_finish (vr_trace.h) built for the host, with and without the shortcut for blocked
shadow rays; the gathers' two addressing forms and the rule that chooses between them.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common

_libs = {}


def build(shortcut=True):
    return hk_common.build(__file__, "hotpair_host.cpp", "libhotpair_host.so" if shortcut else "libhotpair_host_noshortcut.so",
                           ("-Wno-unknown-pragmas",) + (() if shortcut else ("-DVR_SHADOW_BLOCKED_SHORTCUT=0",)))


def lib(shortcut=True):
    if shortcut not in _libs:
        L = C.CDLL(build(shortcut))
        L.hc_shadow_collide.argtypes = [C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
        L.hc_largest_table_bytes.restype = C.c_ulonglong
        L.hc_largest_table_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.hc_addressing_forms_differ.restype = C.c_longlong
        assert L.hc_shortcut_compiled() == (1 if shortcut else 0)
        _libs[shortcut] = L
    return _libs[shortcut]


def shadow_collide(form, states, shortcut=True):
    """states: [n][5] uint32 = RNG state, cell majorant, vol_majorant, Tr, density (floats as bits) -> [n][5] = Tr, state, RNG state, tau, mipq"""
    states = np.ascontiguousarray(states, np.uint32).reshape(-1, 5)
    out = np.zeros_like(states)
    assert lib(shortcut).hc_shadow_collide(int(form), states.shape[0], states.ctypes.data, out.ctypes.data) == 0
    return out


def largest_table_bytes(nb=(1, 1, 1), mshift=(3, 3, 3), dim=(0, 0, 0), float_atlas=False, paired=False, tf=False):
    """vr_scene.h grid_largest_table_bytes of a brick grid of nb bricks, or -- dim given -- of a dense grid of dim voxels"""
    a, b, c = (np.array(v, np.int32) for v in (nb, mshift, dim))
    return int(lib().hc_largest_table_bytes(a.ctypes.data, b.ctypes.data, c.ctypes.data, 1 if any(dim) else 0, int(float_atlas), int(paired), int(tf)))


def addressing_forms_differ(records, cells):
    return int(lib().hc_addressing_forms_differ(int(records), int(cells)))
