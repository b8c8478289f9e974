"""ctypes binding of tests/hostkernel/libvariant_host.so: the product's rule for which compiled path-tracing kernel serves a scene (vr_variant.h) built
for the host.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_common
from hk_common import _p

_lib = None

ANSWER = ("variant", "reason", "instance", "item_integrator", "samples_per_unit", "wide", "reads_seed_table", "scene_reasons", "pairs")


class Grid(C.Structure):
    _fields_ = [("dense", C.c_int32), ("atlas_f32", C.c_int32), ("maj_blocked", C.c_int32), ("nb", C.c_int32 * 3), ("mshift", C.c_int32 * 3),
                ("dim", C.c_int32 * 3), ("dblk", C.c_int32 * 2)]


class Scene(C.Structure):
    _fields_ = [("integrator", C.c_int32), ("use_tf", C.c_int32), ("has_emission", C.c_int32), ("env_div_safe", C.c_int32), ("paired", C.c_int32),
                ("density_scale", C.c_float), ("density", Grid), ("emission", Grid)]


def build():
    return hk_common.build(__file__, "variant_host.cpp", "libvariant_host.so")


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def brick_grid(nb=(4, 4, 4), mshift=(3, 3, 3), atlas_f32=False, maj_blocked=False):
    g = Grid(atlas_f32=int(atlas_f32), maj_blocked=int(maj_blocked))
    g.nb[:] = nb
    g.mshift[:] = mshift
    return g


def dense_grid(dim=(32, 32, 32), nb=(4, 4, 4), mshift=(3, 3, 3)):
    g = brick_grid(nb, mshift)
    g.dense = 1
    g.dim[:] = dim
    g.dblk[:] = [(dim[0] + 3) // 4, (dim[1] + 3) // 4]
    return g


def scene(density, emission=None, paired=0, integrator=0, use_tf=0, env_div_safe=1, density_scale=1.0):
    s = Scene(integrator=integrator, use_tf=use_tf, has_emission=int(emission is not None), env_div_safe=env_div_safe, paired=paired,
              density_scale=float(np.float32(density_scale)), density=density)
    if emission is not None:
        s.emission = emission
    return s


def kernel_of(s, force_wide=False, instrumented=False):
    """{name: value} of ANSWER for the scene"""
    out = np.zeros(len(ANSWER), np.int32)
    lib().vh_kernel_of(C.byref(s), int(force_wide), int(instrumented), _p(out))
    return dict(zip(ANSWER, (int(v) for v in out)))
