"""ctypes binding of tests/hostkernel/libcollide_tail_host.so: collide_finish (vr_trace.h) built for the host in both of its orders.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(hk_common.build(__file__, "collide_tail_host.cpp", "libcollide_tail_host.so", ("-Wno-unknown-pragmas",)))
        L.ct_collide.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
        assert L.ct_shortcut_compiled() == 1
        _lib = L
    return _lib


def collide(tf, early, states):
    """states: [n][9] uint32 = RNG state, cell majorant, vol_majorant, Tr, density or alpha, shadow, mipq, tau, t (floats as bits)
    -> [n][10] = state, RNG state, tau, t, Tr, mipq, majorant, collision colour x 3"""
    states = np.ascontiguousarray(states, np.uint32).reshape(-1, 9)
    out = np.zeros((states.shape[0], 10), np.uint32)
    assert lib().ct_collide(int(tf), int(early), states.shape[0], states.ctypes.data, out.ctypes.data) == 0
    return out
