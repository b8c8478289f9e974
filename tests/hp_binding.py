"""ctypes binding of tests/hostkernel/libprobehost.so: the lookup probes of volren_amd/csrc/vr_probe.h built for the host.
TEST HARNESS ONLY -- lets the CPU-only suite hold every scene-data accessor of the device code to the oracle."""
import ctypes as C

import numpy as np

import hk_binding as hk
import hk_common

MAJ_BLOCKED, NO_FLOAT_ATLAS, NO_COMPACT_ENV, PAIR = 1, 2, 4, 8
VOXEL, TRILINEAR, MAJORANT, IMPORTANCE, TEXEL, SKY, LIGHT, TF = range(8)
OUT_WORDS = (1, 1, 1, 1, 3, 3, 7, 4)


def build(sanitize=False):
    return hk_common.build(__file__, "probe_host.cpp", "libprobehost_san.so" if sanitize else "libprobehost.so",
                           ("-fopenmp", "-Wno-unknown-pragmas") + (hk_common.UBSAN if sanitize else ()))


_libs = {}


def lib(sanitize=False):
    if sanitize not in _libs:
        L = C.CDLL(build(sanitize))
        L.hp_scene_create.restype = C.c_void_p
        L.hp_scene_free.argtypes = [C.c_void_p]
        L.hp_scene_info.argtypes = [C.c_void_p, C.c_void_p]
        L.hp_scene_table.restype = C.c_void_p
        L.hp_scene_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.hp_probe.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_char_p, C.c_int]
        L.hp_pack_texel.argtypes = [C.c_void_p, C.c_void_p]
        L.hp_pack_map.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
        L.hp_unpack_texels.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
        _libs[sanitize] = L
    return _libs[sanitize]


class Refused(Exception):
    """The scene cannot serve the form (vr_probe.h probe_form_error), or an item is out of a table's range."""


class Scene:
    """The scene of an oracle.binding.OracleRenderer as the device code sees it, built by tests/hostkernel/host_scene.h."""

    def __init__(self, orc_renderer, flags=0, sanitize=False):
        self._L = lib(sanitize)
        p = orc_renderer.params()
        assert C.sizeof(p) == self._L.hp_uniforms_size()
        dd = hk.grid_desc(orc_renderer.density)
        ed = hk.grid_desc(orc_renderer.emission) if orc_renderer.emission is not None else None
        env, lut = orc_renderer.env_tex, orc_renderer.lut
        self._keep = (orc_renderer, dd, ed, env, lut, orc_renderer.impmap)
        self._h = self._L.hp_scene_create(C.byref(p), C.byref(dd), C.byref(ed) if ed is not None else None,
                                          lut.ctypes.data_as(C.c_void_p) if lut is not None else None,
                                          env.ctypes.data_as(C.c_void_p), env.shape[1], env.shape[0],
                                          orc_renderer.impmap.ctypes.data_as(C.c_void_p), 512, int(flags))
        info = (C.c_int * 4)()
        self._L.hp_scene_info(self._h, info)
        self.compact, self.div_safe, self.paired, self.float_atlas = (bool(v) for v in info)

    def close(self):
        if self._h:
            self._L.hp_scene_free(self._h)
            self._h = None

    __del__ = close

    def probe(self, what, form, items):
        items = np.ascontiguousarray(items)
        assert items.ndim == 2 and items.shape[1] == 4 and items.dtype.itemsize == 4
        out = np.empty((items.shape[0], OUT_WORDS[what]), np.float32)
        err = C.create_string_buffer(256)
        if self._L.hp_probe(self._h, what, form, items.ctypes.data, out.ctypes.data, items.shape[0], err, 256) != 0:
            raise Refused(err.value.decode())
        return out

    def table(self, which, dtype):
        """A writable view of one of the harness's tables (0 paired atlas, 1 warp table, 2 float majorants, 3 fp16 majorants, 4 compact map)."""
        n = C.c_longlong()
        ptr = self._L.hp_scene_table(self._h, which, C.byref(n))
        if not ptr or n.value == 0:
            return np.zeros(0, dtype)
        nbytes = n.value * np.dtype(dtype).itemsize
        return np.frombuffer((C.c_char * nbytes).from_address(ptr), dtype=dtype)


def pack_texel(rgb):
    """env_pack.h pack_rgbe_texel: the dword, or None when the texel has no compact form."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    q = C.c_uint32()
    return int(q.value) if lib().hp_pack_texel(rgb.ctypes.data, C.byref(q)) else None


def pack_map(tex):
    tex = np.ascontiguousarray(tex, np.float32).reshape(-1, 3)
    out = np.empty(tex.shape[0], np.uint32)
    return out if lib().hp_pack_map(tex.ctypes.data, tex.shape[0], out.ctypes.data) else None


def unpack_texels(q):
    q = np.ascontiguousarray(q, np.uint32)
    out = np.empty((q.size, 3), np.float32)
    lib().hp_unpack_texels(q.ctypes.data, q.size, out.ctypes.data)
    return out
