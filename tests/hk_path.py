"""ctypes binding of tests/hostkernel/libpathprobehost.so: the per-path probes of volren_amd/csrc/vr_path_probe.h built for the host, with the
range-checking trace sink of tests/hostkernel/path_probe_host.cpp.  TEST HARNESS ONLY."""
import ctypes as C

import numpy as np

import hk_binding as hk
import hk_common

MAJ_BLOCKED, NO_FLOAT_ATLAS, NO_COMPACT_ENV, PAIR = 1, 2, 4, 8
RNG, CAMERA, BOX, PHASE, DDA, SEGMENT = range(6)
IN_WORDS = (8, 4, 6, 9, 7, 8)
OUT_WORDS = (5, 4, 3, 5, 1, 14)


def build():
    return hk_common.build(__file__, "path_probe_host.cpp", "libpathprobehost.so", ("-fopenmp", "-Wno-unknown-pragmas", "-DVR_HOST_TRACE"))


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hpp_scene_create.restype = C.c_void_p
        L.hpp_scene_free.argtypes = [C.c_void_p]
        L.hpp_scene_info.argtypes = [C.c_void_p, C.c_void_p]
        L.hpp_constants.argtypes = [C.c_void_p]
        L.hpp_violations.restype = L.hpp_accesses.restype = C.c_longlong
        L.hpp_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
        _lib = L
    return _lib


def constants():
    """(the device code's segment budget, its bound on the passes of one item)"""
    out = (C.c_int * 2)()
    lib().hpp_constants(out)
    return int(out[0]), int(out[1])


def violations():
    """accesses of the lane code outside the table they name, over every probe run so far"""
    return int(lib().hpp_violations())


def accesses():
    return int(lib().hpp_accesses())


class Refused(Exception):
    """The scene cannot serve the form (vr_path_probe.h path_probe_form_error), or a bad item."""


class Scene:
    """The scene of an oracle.binding.OracleRenderer as the device code sees it, built by tests/hostkernel/host_scene.h."""

    def __init__(self, orc_renderer, flags=0):
        self._L = lib()
        p = orc_renderer.params()
        assert C.sizeof(p) == self._L.hpp_uniforms_size()
        dd = hk.grid_desc(orc_renderer.density)
        ed = hk.grid_desc(orc_renderer.emission) if orc_renderer.emission is not None else None
        env, lut = orc_renderer.env_tex, orc_renderer.lut
        self._keep = (orc_renderer, dd, ed, env, lut, orc_renderer.impmap)
        self._h = self._L.hpp_scene_create(C.byref(p), C.byref(dd), C.byref(ed) if ed is not None else None,
                                           lut.ctypes.data_as(C.c_void_p) if lut is not None else None,
                                           env.ctypes.data_as(C.c_void_p), env.shape[1], env.shape[0],
                                           orc_renderer.impmap.ctypes.data_as(C.c_void_p), 512, int(flags))
        info = (C.c_int * 4)()
        self._L.hpp_scene_info(self._h, info)
        self.paired, self.float_atlas, self.instance, self.reason = bool(info[0]), bool(info[1]), int(info[2]), int(info[3])

    def close(self):
        if self._h:
            self._L.hpp_scene_free(self._h)
            self._h = None

    __del__ = close

    def path_probe(self, kind, form, items):
        items = np.ascontiguousarray(items)
        assert items.ndim == 2 and items.shape[1] == IN_WORDS[kind] and items.dtype.itemsize == 4
        out = np.zeros((items.shape[0], OUT_WORDS[kind]), np.uint32)
        err = C.create_string_buffer(256)
        if self._L.hpp_probe(self._h, kind, form, items.ctypes.data, out.ctypes.data, items.shape[0], err, 256) != 0:
            raise Refused(err.value.decode())
        return out
