"""ctypes binding of tests/hostkernel/libhostkernel.so: the product's device code (vr_trace.h) built for the host.
TEST HARNESS ONLY -- lets the CPU-only suite check the lane state machine against the oracle."""
import ctypes as C
import os

import numpy as np

import hk_common


def build(sanitize=False, fast_tap=False):
    """fast_tap: the device's decision of the stochastic-filter tests (VR_TAP_FAST, vr_trace.h) instead of the reference's loop."""
    assert not (sanitize and fast_tap), "there is no sanitizer build of the fast-tap form"
    name, extra = ("libhostkernel_san.so", hk_common.UBSAN) if sanitize else ("libhostkernel_fasttap.so", ("-DVR_TAP_FAST=1",)) if fast_tap else ("libhostkernel.so", ())
    return hk_common.build(__file__, "host_kernel.cpp", name, ("-Wno-unknown-pragmas",) + extra)


def build_tricubic_band_tool():
    """tests/tools_tricubic_band.cpp: exhaustive / strided check of the fast filter tests against the reference's."""
    return hk_common.build(__file__, os.path.join(hk_common.TESTS, "tools_tricubic_band.cpp"), "tricubic_band", ("-fopenmp", "-Wno-unknown-pragmas"), shared=False)


class GridDesc(C.Structure):
    _fields_ = [("nb", C.c_uint32 * 3), ("atlas_dim", C.c_uint32 * 3), ("n_mips", C.c_int32),
                ("indirection", C.c_void_p), ("range", C.c_void_p), ("atlas", C.c_void_p), ("mips", C.c_void_p * 3),
                ("dense", C.c_void_p), ("dim", C.c_uint32 * 3)]


def grid_desc(g):
    d = GridDesc()
    d.nb[:] = g.n_bricks
    d.atlas_dim[:] = g.atlas_dim
    d.n_mips = len(g.mips)
    d.indirection = g.indirection.ctypes.data
    d.range = g.range.ctypes.data
    d.atlas = g.atlas.ctypes.data
    for i, (_, a) in enumerate(g.mips):
        d.mips[i] = a.ctypes.data
    if getattr(g, "dense", None) is not None:
        d.dense = g.dense.ctypes.data
        d.dim[:] = g.extent
    return d


_libs = {}


def lib(fast_tap=False):
    if fast_tap not in _libs:
        L = C.CDLL(build(fast_tap=fast_tap))
        L.hk_render.restype = C.c_longlong
        L.hk_render_tiles.restype = C.c_longlong
        L.hk_math.restype = C.c_float
        L.hk_math.argtypes = [C.c_int, C.c_float, C.c_float]
        _libs[fast_tap] = L
    return _libs[fast_tap]


# The forms of the lane code the harness compiles: exactly the 14 configurations the device ships (host_kernel.cpp FormCfg, vr_pathtrace.hip Cfg), in the
# order of the product's instances (vr_variant.h PathtraceKernel::instance; form = 2 * instance + tf): (kernel variant, 64-bit gather addresses, transfer function)
FORMS = tuple((variant, wide, tf) for variant, wide in ((0, False), (0, True), (1, False), (1, True), (2, True), (4, True), (3, True)) for tf in (False, True))
# host_kernel.cpp g_form_steps: the first five as they always were; then the lane steps by the state they were entered in -- what the device's instrumented
# instances count as the lanes of a block --, the transitions that end a path or an item, and what relates a march pass to the reference's DDA iterations
COUNTERS = ("steps", "clean_march", "clean_collide", "general_march", "general_collide",
            "new", "march", "collide", "nee", "postnee", "escape",
            "ended", "outside", "new_escape", "primary_miss", "march_dda", "march_empty", "shadow_segments")
HS_MAJ_BLOCKED = 1            # host_scene.h


def form_steps(reset=False, fast_tap=False):
    """{form: {counter: n}} since the last reset, forms as in FORMS: all lane steps, and the steps of the hot pair by what the path stood on -- a clean segment
    (vr_trace.h seg_clean) or not, which is where lane_step takes the general forms -- counted by the harness before each step."""
    L = lib(fast_tap)
    assert L.hk_form_count() == len(FORMS)
    out = (C.c_ulonglong * (len(FORMS) * len(COUNTERS)))()
    L.hk_form_steps(out, 1 if reset else 0)
    return {f: {c: int(out[i * len(COUNTERS) + k]) for k, c in enumerate(COUNTERS)} for i, f in enumerate(FORMS)}


def forms_that_ran(fast_tap=False):
    """{form: lane steps} of the forms with a step since the last reset"""
    return {f: c["steps"] for f, c in form_steps(fast_tap=fast_tap).items() if any(c.values())}


def render(orc_renderer, spp, rect=None, fb=None, first_sample=1, fast_tap=False, wide=False, blocked=False):
    """Run the host-compiled product kernel on the scene held by an oracle.binding.OracleRenderer, in the form the product's launch would pick for it
    (vr_variant.h pathtrace_kernel_of, which the harness calls).  wide: the 64-bit form of variants 0 and 1 (the product's wide_addressing = 1);
    blocked: majorant levels 0-1 in 4x4x4-cell blocks where the product has a kernel for them (majorant_layout = 1: variant 4 instead of 2)."""
    L = lib(fast_tap)
    p = orc_renderer.params()
    assert C.sizeof(p) == L.hk_uniforms_size(), (C.sizeof(p), L.hk_uniforms_size())
    dd = grid_desc(orc_renderer.density)
    ed = grid_desc(orc_renderer.emission) if orc_renderer.emission is not None else None
    w, h = orc_renderer.w, orc_renderer.h
    if fb is None:
        fb = np.zeros((h, w, 4), np.float32)
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w, h)
    env = orc_renderer.env_tex
    lut = orc_renderer.lut
    steps = L.hk_render(C.byref(p), C.byref(dd), C.byref(ed) if ed is not None else None,
                        lut.ctypes.data_as(C.c_void_p) if lut is not None else None,
                        env.ctypes.data_as(C.c_void_p), env.shape[1], env.shape[0],
                        orc_renderer.impmap.ctypes.data_as(C.c_void_p), 512,
                        fb.ctypes.data_as(C.c_void_p), x0, y0, x1, y1, first_sample, spp, 1 if wide else 0, HS_MAJ_BLOCKED if blocked else 0)
    assert steps >= 0
    return fb, steps


def render_tiles(orc_renderer, spp, tiles=None, fb=None, first_sample=1, fast_tap=False, wide=False, blocked=False):
    """The same scene walked as the device walks a launch (host_kernel.cpp hk_render_tiles): every item of every listed 16x16 tile (raster ids, row 0 = bottom;
    None: all tiles of the frame), the items outside a ragged frame included.  Returns (frame, lane steps)."""
    L = lib(fast_tap)
    p = orc_renderer.params()
    assert C.sizeof(p) == L.hk_uniforms_size(), (C.sizeof(p), L.hk_uniforms_size())
    dd = grid_desc(orc_renderer.density)
    ed = grid_desc(orc_renderer.emission) if orc_renderer.emission is not None else None
    if fb is None:
        fb = np.zeros((orc_renderer.h, orc_renderer.w, 4), np.float32)
    t = np.ascontiguousarray(tiles, np.int32) if tiles is not None else None
    env = orc_renderer.env_tex
    lut = orc_renderer.lut
    steps = L.hk_render_tiles(C.byref(p), C.byref(dd), C.byref(ed) if ed is not None else None,
                              lut.ctypes.data_as(C.c_void_p) if lut is not None else None,
                              env.ctypes.data_as(C.c_void_p), env.shape[1], env.shape[0],
                              orc_renderer.impmap.ctypes.data_as(C.c_void_p), 512,
                              fb.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p) if t is not None else None, int(t.size) if t is not None else 0,
                              first_sample, spp, 1 if wide else 0, HS_MAJ_BLOCKED if blocked else 0)
    assert steps >= 0, steps
    return fb, steps
