"""Python mirror of the reference's Renderer object (src/renderer.h:16-63 as exposed by src/bindings.cpp:117-209),
backed by the HIP library through its C ABI.  Attribute names are the reference's field names."""
import ctypes as C

import numpy as np

from . import _lib

_INT_FIELDS = ("sample", "sppx", "seed", "bounces", "show_environment", "tonemapping", "integrator", "grid_frame_counter",
               "sample_pool_mb", "gpu_encoder", "fast_math", "tf_float_atlas", "launch_target_ms", "order_tiles", "coalesce_trace", "majorant_layout",
               "variance", "denoise_iterations", "denoise_moments", "denoise_resolve", "denoise_layers", "denoise_filter", "denoise_demodulate", "wide_addressing", "seed_table_mb", "seed_table_max_samples",
               "expected_skip", "expected_field", "expected_stats", "sky_tiles", "see_through_tiles")
_READ_ONLY_INT_FIELDS = ("n_grid_frames", "last_launches", "last_sky_tiles", "last_see_through_tiles", "pending_samples", "majorant_blocked", "env_div_safe", "env_compact", "kernel_variant", "kernel_variant_reason",
                         "kernel_wide", "adaptive_rounds", "seed_table_samples", "seed_table_fills")
_FLOAT_FIELDS = {"tonemap_exposure": 1, "tonemap_gamma": 1, "albedo": 3, "phase": 1, "density_scale": 1,
                 "emission_scale": 1, "vol_clip_min": 3, "vol_clip_max": 3, "env_strength": 1, "env_transform": 9,
                 "tf_window_left": 1, "tf_window_width": 1, "cam_pos": 3, "cam_dir": 3, "cam_up": 3, "cam_fov": 1,
                 "volume_transform": 16, "denoise_sigma": 5, "denoise_alpha": 1, "denoise_reject": 1, "denoise_ridge": 1}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Renderer:
    """`Renderer(w, h)`; set fields; `load_volume/load_envmap/load_transferfunc`; `render(spp)`; `fbo_data()`.

    One name is both a field and a method: `r.variance = 1` switches the per-pixel moments on (vr_set_int "variance"), `r.variance()` returns the
    variance buffer, and `r.get_int("variance")` reads the switch back (the attribute itself is the method)."""

    def __init__(self, width, height, device=0, _borrowed=None):
        object.__setattr__(self, "_h", None)
        L = _lib.load()
        object.__setattr__(self, "_owned", _borrowed is None)
        if _borrowed is None:
            h = C.c_void_p()
            _lib.check(L.vr_create(C.byref(h), int(device), int(width), int(height)))
        else:
            h = C.c_void_p(_borrowed)                       # a part of a ShardedRenderer: the handle belongs to it
        object.__setattr__(self, "_h", h)
        object.__setattr__(self, "_L", L)
        object.__setattr__(self, "width", int(width))
        object.__setattr__(self, "height", int(height))

    def close(self):
        if self._h is not None:
            if self._owned:
                self._L.vr_destroy(self._h)
            object.__setattr__(self, "_h", None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- fields ----
    def get_int(self, name):
        """vr_get_int: an int field by name (e.g. "variance", whose attribute name is taken by the method variance())."""
        v = C.c_int()
        _lib.check(self._L.vr_get_int(self._h, name.encode(), C.byref(v)))
        return v.value

    def __getattr__(self, name):
        if name in _INT_FIELDS or name in _READ_ONLY_INT_FIELDS:
            v = self.get_int(name)
            return bool(v) if name in ("show_environment", "tonemapping") else v
        if name in _FLOAT_FIELDS:
            n = _FLOAT_FIELDS[name]
            buf = (C.c_float * n)()
            _lib.check(self._L.vr_get_float(self._h, name.encode(), buf, n))
            return buf[0] if n == 1 else np.array(buf[:], np.float32)
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _INT_FIELDS:
            _lib.check(self._L.vr_set_int(self._h, name.encode(), int(value)))
        elif name in _FLOAT_FIELDS or name == "env_rot":
            v = _f32(np.atleast_1d(value)).reshape(-1)
            _lib.check(self._L.vr_set_float(self._h, name.encode(), v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
        else:
            object.__setattr__(self, name, value)

    def has_fast_math(self):
        """The library carries the opt-in tolerance-mode kernels (`fast_math = 1`); the default kernels are bit-exact."""
        return True

    # ---- scene ----
    def load_volume(self, path):
        _lib.check(self._L.vr_load_volume(self._h, str(path).encode()))

    def set_volume_path(self, path):
        """`renderer.volume = Volume(path)` of the reference's Python module: replaces the volume only (no commit)."""
        _lib.check(self._L.vr_set_volume_path(self._h, str(path).encode()))

    def volume_aabb(self, name="density"):
        out = (C.c_float * 6)()
        _lib.check(self._L.vr_volume_aabb(self._h, name.encode(), out))
        return np.array(out[:3], np.float32), np.array(out[3:], np.float32)

    def volume_minorant_majorant(self, name="density"):
        out = (C.c_float * 2)()
        _lib.check(self._L.vr_volume_minorant_majorant(self._h, name.encode(), out))
        return float(out[0]), float(out[1])

    def load_envmap(self, path):
        _lib.check(self._L.vr_load_envmap(self._h, str(path).encode()))

    def load_transferfunc(self, path):
        _lib.check(self._L.vr_load_transferfunc(self._h, str(path).encode()))

    def set_volume_dense(self, voxels_zyx, transform=None, name="density", unit_cube=True, commit=True):
        v = _f32(voxels_zyx)
        nz, ny, nx = v.shape
        t = _f32(transform).reshape(16) if transform is not None else None
        _lib.check(self._L.vr_set_volume_dense(self._h, name.encode(), v.ctypes.data, nx, ny, nz,
                                               t.ctypes.data if t is not None else None, 1 if unit_cube else 0))
        if commit:
            self.commit()

    def volume_add_grid_frame(self, voxels_zyx, name="density", transform=None):
        """voldata::Volume::add_grid_frame: one more animation frame holding the dense grid `name` (commit() afterwards)."""
        v = _f32(voxels_zyx)
        nz, ny, nx = v.shape
        t = _f32(transform).reshape(16) if transform is not None else None
        _lib.check(self._L.vr_volume_add_grid_frame_dense(self._h, name.encode(), v.ctypes.data, nx, ny, nz, t.ctypes.data if t is not None else None))

    def volume_update_grid_frame(self, frame, voxels_zyx, name="density", transform=None):
        """voldata::Volume::update_grid_frame: grid `name` of frame `frame` replaced (commit() afterwards)."""
        v = _f32(voxels_zyx)
        nz, ny, nx = v.shape
        t = _f32(transform).reshape(16) if transform is not None else None
        _lib.check(self._L.vr_volume_update_grid_frame_dense(self._h, int(frame), name.encode(), v.ctypes.data, nx, ny, nz, t.ctypes.data if t is not None else None))

    def volume_n_grid_frames(self):
        n = C.c_int()
        _lib.check(self._L.vr_volume_n_grid_frames(self._h, C.byref(n)))
        return n.value

    def set_volume_dense_f16(self, voxels_zyx, transform=None, name="density", unit_cube=True, commit=True):
        """Dense fp16 grid kept dense on the device (2 B/voxel, no brick indirection)."""
        v = np.ascontiguousarray(voxels_zyx, dtype=np.float16)
        nz, ny, nx = v.shape
        t = _f32(transform).reshape(16) if transform is not None else None
        _lib.check(self._L.vr_set_volume_dense_f16(self._h, name.encode(), v.ctypes.data, nx, ny, nz,
                                                   t.ctypes.data if t is not None else None, 1 if unit_cube else 0))
        if commit:
            self.commit()

    def set_volume_brick(self, transform, n_bricks, min_maj, indirection, rng, atlas_dim, atlas, mips=(), name="density",
                         unit_cube=True, commit=True):
        t = _f32(transform).reshape(16)
        nb = np.asarray(n_bricks, np.uint32)
        mm = _f32(min_maj)
        ind = np.ascontiguousarray(indirection, np.uint32)
        rg = np.ascontiguousarray(rng, np.uint32)
        ad = np.asarray(atlas_dim, np.uint32)
        at = np.ascontiguousarray(atlas, np.uint8)
        mip_arrays = [np.ascontiguousarray(a, np.uint32) for _, a in mips]
        mip_ptrs = (C.c_void_p * max(1, len(mips)))(*[a.ctypes.data for a in mip_arrays])
        mip_dims = np.asarray([d for d, _ in mips], np.uint32).reshape(-1, 3) if mips else np.zeros((1, 3), np.uint32)
        _lib.check(self._L.vr_set_volume_brick(self._h, name.encode(), t.ctypes.data, nb.ctypes.data, mm.ctypes.data,
                                               ind.ctypes.data, rg.ctypes.data, ad.ctypes.data, at.ctypes.data,
                                               len(mips), C.cast(mip_ptrs, C.c_void_p), mip_dims.ctypes.data, 1 if unit_cube else 0))
        if commit:
            self.commit()

    def set_envmap(self, rgb_top_first):
        a = _f32(rgb_top_first)
        _lib.check(self._L.vr_set_envmap(self._h, a.ctypes.data, a.shape[1], a.shape[0]))

    def set_transferfunc(self, lut):
        if lut is None:
            _lib.check(self._L.vr_set_transferfunc(self._h, None, 0))
            return
        a = _f32(lut)
        _lib.check(self._L.vr_set_transferfunc(self._h, a.ctypes.data, a.shape[0]))

    def commit(self):
        _lib.check(self._L.vr_commit(self._h))

    def reset(self):
        _lib.check(self._L.vr_reset(self._h))

    def resize(self, w, h):
        _lib.check(self._L.vr_resize(self._h, int(w), int(h)))
        object.__setattr__(self, "width", int(w))
        object.__setattr__(self, "height", int(h))

    def scale_and_move_to_unit_cube(self):
        _lib.check(self._L.vr_scale_and_move_to_unit_cube(self._h))

    # ---- rendering ----
    def trace(self):
        """One more sample (RendererOpenGL::trace).  Consecutive calls on an unchanged scene are launched together (include/volren_amd.h)."""
        _lib.check(self._L.vr_trace(self._h))

    def flush(self):
        """Launch the samples recorded by trace() without waiting for them."""
        _lib.check(self._L.vr_flush(self._h))

    def render(self, spp=0, sync=True):
        """`spp` more samples per pixel in one fused launch (the reference loops trace(); bindings.cpp:124-132)."""
        _lib.check(self._L.vr_render(self._h, int(spp)))
        if sync:
            self.synchronize()

    def synchronize(self):
        _lib.check(self._L.vr_synchronize(self._h))

    def last_kernel_ms(self):
        ms = C.c_double()
        _lib.check(self._L.vr_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_pathtrace_ms(self):
        """HIP-event duration of the path-tracing kernel alone (last sub-launch; no accumulation pass)."""
        ms = C.c_double()
        _lib.check(self._L.vr_last_pathtrace_ms(self._h, C.byref(ms)))
        return ms.value

    def _read_back(self, fn, *trailing, size=None):
        """[H][W] + trailing float32 filled by fn(handle, pointer); size: (W, H) where it is not the renderer's."""
        w, h = size or (self.width, self.height)
        out = np.empty((h, w) + trailing, np.float32)
        _lib.check(fn(self._h, out.ctypes.data))
        return out

    def framebuffer(self):
        """RGBA32F [H][W][4], row 0 = bottom (GL order)."""
        return self._read_back(self._L.vr_framebuffer, 4)

    def fbo_data(self):
        """float RGB of the framebuffer (bindings.cpp:141-148)."""
        return self.framebuffer()[..., :3].copy()

    # ---- test hook ----
    PROBE_OUT_WORDS = (1, 1, 1, 1, 3, 3, 7, 4, 4)   # voxel, trilinear, majorant, importance, texel, sky, light sample, transfer function, cubic (value, gradient)

    def probe(self, what, form, items):
        """Test hook (include/volren_amd.h vr_probe, volren_amd/csrc/vr_probe.h): `items` is [n][4] 32-bit words (int32, uint32 or float32 -- the bits are passed
        as they are); returns [n][k] float32 from the device's own accessors in compile-time form `form`, on the scene as the next launch would read it."""
        items = np.ascontiguousarray(items)
        assert items.ndim == 2 and items.shape[1] == 4 and items.dtype.itemsize == 4, "items: [n][4] 32-bit words"
        out = np.empty((items.shape[0], self.PROBE_OUT_WORDS[int(what)]), np.float32)
        _lib.check(self._L.vr_probe(self._h, int(what), int(form), items.ctypes.data, out.ctypes.data, items.shape[0]))
        return out

    PATH_IN_WORDS = (8, 4, 6, 9, 7, 8)            # RNG, camera ray, box clip, phase / MIS, DDA step, segment
    PATH_OUT_WORDS = (5, 4, 3, 5, 1, 14)

    def path_probe(self, kind, form, items):
        """Test hook (include/volren_amd.h vr_path_probe, volren_amd/csrc/vr_path_probe.h): `items` is [n][PATH_IN_WORDS[kind]] 32-bit words; returns
        [n][PATH_OUT_WORDS[kind]] uint32 (floats as their bits) from the device's own per-path code in form `form` (a segment: the compiled instance)."""
        items = np.ascontiguousarray(items)
        assert items.ndim == 2 and items.shape[1] == self.PATH_IN_WORDS[int(kind)] and items.dtype.itemsize == 4, "items: [n][words] 32-bit words"
        out = np.zeros((items.shape[0], self.PATH_OUT_WORDS[int(kind)]), np.uint32)
        _lib.check(self._L.vr_path_probe(self._h, int(kind), int(form), items.ctypes.data, out.ctypes.data, items.shape[0]))
        return out

    FILTER_STAGES = ("prepare", "atrous", "temporal", "resolve", "split", "merge", "regress", "upsample", "adaptive_error")

    def filter_probe(self, stage, w, h, inputs, outputs, sigma=(4.0, 0.5, 0.1, 0.25, 0.2), i0=0, x=0.0, tau=0.0, i1=0, cur=None, prev=None, demod=False):
        """Test hook (include/volren_amd.h vr_filter_probe): one launcher of the image-space kernels on host arrays.  stage: a name of FILTER_STAGES or its number;
        inputs: up to 6 arrays in the stage's order, float32 (counts and tile ids int32), None where one is left out; outputs: up to 5 shapes in the stage's order,
        None likewise; the rest is the parameter block (cur, prev: cameras of 13 float32; demod: the DEMOD instance of prepare, split, merge, upsample).  Returns the outputs as float32 arrays, None where none was asked for.
        Nothing of the renderer changes."""
        stage = self.FILTER_STAGES.index(stage) if isinstance(stage, str) else int(stage)
        keep = []
        for a in inputs:
            if a is not None:
                a = np.ascontiguousarray(a)
                assert a.dtype in (np.float32, np.int32), "inputs: float32, or int32 for counts and tile ids"
            keep.append(a)
        outs = [None if s is None else np.zeros(s, np.float32) for s in outputs]
        # the sizes the library will read and write (words of 4 bytes): the header's table
        px, hi, tiles, n = int(w) * int(h), int(w) * int(h) * int(i1) ** 2, ((int(w) + 15) // 16) * ((int(h) + 15) // 16), int(i0)
        want_in = ((4 * px, 8 * px, tiles), (4 * px, px, 8 * px), (4 * px, px, 8 * px, 4 * px, 4 * px, 4 * px), (4 * px, 8 * px), (4 * px, 4 * px, 8 * px),
                   (4 * px, 4 * px, 8 * px), (4 * px, 8 * px), (4 * px, 8 * px, 8 * hi), (4 * px, 4 * px, n, n))[stage]
        want_out = ((px, 8 * px), (4 * px, px), (4 * px, 4 * px, px, 4 * px, 4 * px), (4 * px,) * 3, (4 * px,), (4 * px,) * 2, (4 * px,), (4 * hi,) * 2, (n,))[stage]
        assert len(keep) <= len(want_in) and len(outs) <= len(want_out), "more arrays than the stage has"
        assert all(a is None or a.size == k for a, k in zip(keep, want_in)), "an input array is not of the stage's size"
        assert all(o is None or o.size == k for o, k in zip(outs, want_out)), "an output array is not of the stage's size"
        pin = (C.c_void_p * 6)(*([None if a is None else a.ctypes.data for a in keep] + [None] * (6 - len(keep))))
        pout = (C.c_void_p * 5)(*([None if o is None else o.ctypes.data for o in outs] + [None] * (5 - len(outs))))
        p = np.zeros(40, np.float32)
        p[0:5] = sigma
        p[5], p[6], p[7], p[8] = i0, x, tau, i1
        if cur is not None:
            p[9:22] = cur
        if prev is not None:
            p[22:35] = prev
        p[35] = int(demod)
        _lib.check(self._L.vr_filter_probe(self._h, stage, int(w), int(h), pin, pout, p.ctypes.data))
        return outs

    # ---- denoiser data ----
    def render_features(self, spp, sync=True):
        """First-scatter features of samples 1..spp of every pixel (include/volren_amd.h vr_render_features), computed afresh."""
        _lib.check(self._L.vr_render_features(self._h, int(spp)))
        if sync:
            self.synchronize()

    def render_features_expected(self, rays=2, sync=True):
        """The expected values of the same features from rays x rays deterministic ray marches per pixel, rays in 1..4 (include/volren_amd.h
        vr_render_features_expected): no noise, no dependence on spp or seed; fills the buffer features() and the denoiser read.
        `expected_field = 1` marches the field the tracker decides its collisions on (without a LUT the cubic B-spline field) instead of the trilinear one."""
        _lib.check(self._L.vr_render_features_expected(self._h, int(rays)))
        if sync:
            self.synchronize()

    def expected_stats(self, enable=None):
        """Work counters of the expected-value pass (include/volren_amd.h vr_expected_stats).  Like `variance`, the name is a field and a method:
        `r.expected_stats = 1`, or expected_stats(True / False), switches the counting of the following passes on or off (vr_set_int
        "expected_stats"; get_int reads it back); expected_stats() waits and returns the last pass's totals
        {"rays", "steps", "fetched", "reads"}: sub-rays marched, steps reached, steps that fetched their corners, reads of the clear-distance table."""
        if enable is not None:
            _lib.check(self._L.vr_set_int(self._h, b"expected_stats", 1 if enable else 0))
            return None
        out = (C.c_uint64 * 4)()
        _lib.check(self._L.vr_expected_stats(self._h, out))
        return dict(zip(("rays", "steps", "fetched", "reads"), (int(v) for v in out)))

    def expected_clear_table(self):
        """Test hook (vr_expected_clear_table): the clear-distance table of the current density grid that the current `expected_field` marches with,
        uint8 [cz][cy][cx], built if need be."""
        n = (C.c_int * 3)()
        _lib.check(self._L.vr_expected_clear_table(self._h, None, n))
        out = np.empty((n[2], n[1], n[0]), np.uint8)
        _lib.check(self._L.vr_expected_clear_table(self._h, out.ctypes.data, n))
        return out

    def features(self):
        """[H][W][8] float32, row 0 = bottom: albedo.rgb, coverage, normal.xyz, depth."""
        return self._read_back(self._L.vr_features, 8)

    def variance(self):
        """[H][W][4] float32, row 0 = bottom: unbiased per-channel variance of samples 1..sample (needs `variance = 1` for all of them)."""
        return self._read_back(self._L.vr_variance, 4)

    # ---- denoiser ----
    def denoise(self, sync=True):
        """The a-trous filter of the current frame (include/volren_amd.h vr_denoise): needs `variance = 1` for all its samples and a render_features
        since the last resize; `denoise_iterations` / `denoise_sigma` set it up.  `denoise_filter = 1` (default 0; needs `denoise_layers = 1`; a change drops
        the history) runs one 11 x 11 pass of weighted local regression on the scattered layer in the iterations' place (csrc/vr_regress.h); `denoise_ridge`
        is the ridge on its seven slopes, 0 (the default: zero order) or in [2^-20, 2^20].  `denoise_demodulate = 1` (default 0; needs
        `denoise_layers = 1`; a change drops the history) divides the scattered layer by the guide's albedo in front of either filter and multiplies it back
        behind it (csrc/vr_demod.h); upsample() then demodulates the layer it rebuilds as well."""
        _lib.check(self._L.vr_denoise(self._h))
        if sync:
            self.synchronize()

    def denoise_temporal(self, sync=True):
        """denoise() with the frame first blended into the history of the frames before it, reprojected by depth (include/volren_amd.h
        vr_denoise_temporal): once per frame, frames of equal spp; `denoise_alpha` is the smallest weight of the current frame."""
        _lib.check(self._L.vr_denoise_temporal(self._h))
        if sync:
            self.synchronize()

    def denoise_history(self):
        """(colour [H][W][4], variance [H][W], length [H][W]) float32, row 0 = bottom: the history denoise_temporal() keeps."""
        c = np.empty((self.height, self.width, 4), np.float32)
        v = np.empty((self.height, self.width), np.float32)
        n = np.empty((self.height, self.width), np.float32)
        _lib.check(self._L.vr_denoise_history(self._h, c.ctypes.data, v.ctypes.data, n.ctypes.data))
        return c, v, n

    def denoise_reject_stat(self):
        """[H][W] float32, row 0 = bottom: the rejection statistic T of the last denoise_temporal() (a pixel was rejected iff not T <= `denoise_reject`),
        -1 where the pixel had no history.  Needs `denoise_reject` > 0 at that call."""
        return self._read_back(self._L.vr_denoise_reject_stat)

    def denoise_history_moments(self):
        """[H][W][4] float32, row 0 = bottom: the history's moment records (m1, m2, E, S) -- integrated first and second moments of the frames' luminance,
        the sum of squared blend weights, the variance of one frame's luminance.  Needs a history written with `denoise_moments = 1` (a change of that
        field drops the history)."""
        return self._read_back(self._L.vr_denoise_history_moments, 4)

    def denoise_history_reset(self):
        """Drops the history: the next denoise_temporal() starts afresh."""
        _lib.check(self._L.vr_denoise_history_reset(self._h))

    def denoised(self):
        """[H][W][4] float32, row 0 = bottom: the last denoise()'s or denoise_temporal()'s result, linear (not tonemapped)."""
        return self._read_back(self._L.vr_denoised, 4)

    # ---- control variate on the expected coverage ----
    def resolve(self, sync=True):
        """The frame with its hit/miss noise replaced by the expected coverage, y = x + (B - C~)(alpha - kappa) (include/volren_amd.h vr_resolve): needs
        a render_features_expected(rays >= 2) since the last resize, no tile subset, `integrator` != 2; works at any sample count.  `denoise_resolve = 1`
        makes denoise() and denoise_temporal() start from it."""
        _lib.check(self._L.vr_resolve(self._h))
        if sync:
            self.synchronize()

    def resolved(self):
        """[H][W][4] float32, row 0 = bottom: the last resolve()'s result, linear (not tonemapped), alpha = the expected coverage."""
        return self._read_back(self._L.vr_resolved, 4)

    def resolve_background(self):
        """Test hook (vr_resolve_background): [H][W][4] float32, row 0 = bottom: the environment radiance B behind every pixel as the last resolve()
        formed it (0 while `show_environment` is 0), alpha 0."""
        return self._read_back(self._L.vr_resolve_background, 4)

    def denoised_layer(self):
        """[H][W][4] float32, row 0 = bottom: the layer of the last denoise() / denoise_temporal() with `denoise_layers = 1` (include/volren_amd.h
        vr_denoised_layer): the filtered scattered light premultiplied by the exact coverage, alpha = the coverage; over a background B' it composites
        as (1 - a) B' + rgb.  Refused before the first such call since the last resize."""
        return self._read_back(self._L.vr_denoised_layer, 4)

    def upsample(self, factor=2, rays=2):
        """Rebuild the frame at `factor` (2..4) times this renderer's size per axis from the layer of the last denoise() / denoise_temporal() with
        `denoise_layers = 1`, under an expected-value guide of `rays` (1..4) rays per axis marched at the large size (include/volren_amd.h vr_upsample,
        csrc/vr_upsample.h).  Asynchronous.  Keep the camera and the scene as they were at the denoise call.  Refused without such a layer since the last
        resize, after a denoise() / denoise_temporal() with `denoise_layers = 0` (its guide has replaced the layer's) until one with 1 has run again, or with a
        tile subset set.  Results: upsampled(), upsampled_layer(), upsampled_features()."""
        _lib.check(self._L.vr_upsample(self._h, int(factor), int(rays)))

    def upsampled_size(self):
        """(W, H) of the last upsample(); refused before the first one since the last resize."""
        wh = (C.c_int * 2)()
        _lib.check(self._L.vr_upsampled_size(self._h, wh))
        return int(wh[0]), int(wh[1])

    def _upsampled(self, fn, channels):
        return self._read_back(fn, channels, size=self.upsampled_size())

    def upsampled(self):
        """[H][W][4] float32 at the upsampled size, row 0 = bottom: the frame of the last upsample(), alpha = the exact coverage."""
        return self._upsampled(self._L.vr_upsampled, 4)

    def upsampled_layer(self):
        """[H][W][4] float32 at the upsampled size: the scattered light premultiplied by the exact coverage, alpha = the coverage (as denoised_layer())."""
        return self._upsampled(self._L.vr_upsampled_layer, 4)

    def upsampled_features(self):
        """[H][W][8] float32 at the upsampled size: the expected-value feature buffer the last upsample() marched, in features()'s layout."""
        return self._upsampled(self._L.vr_upsampled_features, 8)

    # ---- adaptive sampling ----
    def render_adaptive(self, min_spp, max_spp, threshold, sync=True):
        """Per 16x16 tile: min_spp samples, then doubling until the tile's error e_t is below `threshold` or it has max_spp samples
        (include/volren_amd.h vr_render_adaptive).  Keeps the moments whatever `variance` says; `sample` becomes the largest tile count."""
        _lib.check(self._L.vr_render_adaptive(self._h, int(min_spp), int(max_spp), float(threshold)))
        if sync:
            self.synchronize()

    def _tiles(self):
        return (self.height + 15) // 16, (self.width + 15) // 16

    def tile_samples(self):
        """[tiles_y][tiles_x] int32, row 0 = bottom: the samples behind each tile (`sample` everywhere on a uniform frame)."""
        out = np.empty(self._tiles(), np.int32)
        _lib.check(self._L.vr_tile_samples(self._h, out.ctypes.data, out.size))
        return out

    def tile_error(self):
        """[tiles_y][tiles_x] float32, row 0 = bottom: e_t of each tile at its current count (needs moments that cover the frame)."""
        out = np.empty(self._tiles(), np.float32)
        _lib.check(self._L.vr_tile_error(self._h, out.ctypes.data, out.size))
        return out

    def framebuffer_device_ptr(self):
        p = C.c_void_p()
        _lib.check(self._L.vr_framebuffer_device(self._h, C.byref(p)))
        return p.value

    def draw(self):
        _lib.check(self._L.vr_draw(self._h))

    def display(self):
        return self._read_back(self._L.vr_display, 4)

    def save(self, path):
        _lib.check(self._L.vr_save_png(self._h, str(path).encode()))

    # ---- additions ----
    def set_tiles(self, tile_ids):
        t = np.ascontiguousarray(tile_ids, np.int32)
        _lib.check(self._L.vr_set_tiles(self._h, t.ctypes.data if t.size else None, int(t.size)))

    def set_stream(self, stream_handle):
        _lib.check(self._L.vr_set_stream(self._h, C.c_void_p(stream_handle)))

    def pack_tiles(self, tile_ids_dev_ptr, n, packed_dev_ptr):
        _lib.check(self._L.vr_pack_tiles(self._h, C.c_void_p(tile_ids_dev_ptr), int(n), C.c_void_p(packed_dev_ptr)))

    def unpack_tiles(self, tile_ids_dev_ptr, n, packed_dev_ptr):
        _lib.check(self._L.vr_unpack_tiles(self._h, C.c_void_p(tile_ids_dev_ptr), int(n), C.c_void_p(packed_dev_ptr)))

    def uniforms_bytes(self):
        n = self._L.vr_uniforms_size()
        buf = (C.c_uint8 * n)()
        _lib.check(self._L.vr_get_uniforms(self._h, buf, n))
        return bytes(buf)

    def set_sched(self, thresholds):
        """Scheduler thresholds of THIS renderer's launches (8 ints: vr::PathtraceTuning::thr, csrc/vr_device.h)."""
        t = np.ascontiguousarray(thresholds, np.int32)
        assert t.size == 8
        _lib.check(self._L.vr_set_sched(self._h, t.ctypes.data))

    def sched_stats(self, enable=True, read=False):
        """Scheduler diagnostics of this renderer's path-tracing launches. Returns {state: (executions, active_lanes)} when read."""
        out = np.zeros(32, np.uint64) if read else None
        _lib.check(self._L.vr_sched_stats(self._h, 1 if enable else 0, out.ctypes.data if read else None))
        if not read:
            return None
        d = {n: (int(out[2 * i]), int(out[2 * i + 1])) for i, n in enumerate(STATE_NAMES)}
        d["resumes"], d["parks"] = int(out[14]), int(out[15])      # iterations in which the resume / the park block ran
        d["iterations"] = int(out[16])
        d["waves"] = int(out[17])
        d["cycles"] = {n: int(out[18 + i]) for i, n in enumerate(STATE_NAMES)}     # shader-clock ticks inside each state's block
        d["wave_cycles"] = int(out[25])                                            # summed lifetime of all wavefronts
        d["occupancy"] = {n: int(out[26 + i]) / max(1, int(out[16])) for i, n in enumerate(("marching", "ready", "nee", "postnee", "escape", "free"))}
        d["raw"] = [int(v) for v in out]                                           # the 32 words as the kernels summed them (csrc/vr_pathtrace.h lds_stat)
        return d

    def wave_timeline(self, n_waves=8192):
        """(begin, queue empty, end) per wavefront of the last instrumented launch, in seconds relative to the earliest begin; rows of wavefronts that did not run are dropped."""
        out = np.zeros(3 * n_waves, np.uint64)
        _lib.check(self._L.vr_wave_timeline(self._h, out.ctypes.data, out.size))
        t = out.reshape(-1, 3)
        t = t[t[:, 2] > 0].astype(np.float64)
        t0 = t[:, 0].min() if len(t) else 0.0
        t[:, 1] = np.where(t[:, 1] > 0, t[:, 1], t[:, 2])
        return (t - t0) / 1e8

    def grid_checksums(self):
        out = (C.c_uint64 * 3)()
        _lib.check(self._L.vr_grid_checksums(self._h, out))
        return tuple(int(v) for v in out)

    def impmap(self):
        n = self._L.vr_impmap_floats(self._h)
        out = np.empty(n, np.float32)
        _lib.check(self._L.vr_get_impmap(self._h, out.ctypes.data, n))
        return out


def _part0(name, settable, doc):
    """A ShardedRenderer attribute that reads part 0's field `name`; settable: writing it writes every part's."""
    def fget(self):
        return getattr(self.parts[0], name)

    def fset(self, value):
        for p in self.parts:
            setattr(p, name, value)
    return property(fget, fset if settable else None, doc=doc)


class ShardedRenderer:
    """One frame on several devices in ONE process (include/volren_amd.h vr_sharded_*, csrc/sharded.h): `parts[i]` is an ordinary
    Renderer on `devices[i]` -- replicate the scene by applying the same calls to every part (`each`) -- `render(spp)` lets every
    part render its diagonal share of the 16x16 tiles and gathers them (RCCL all-gather between distinct devices, device-to-device
    copies between logical shards of one device); afterwards `parts[0]` holds the whole frame."""

    def __init__(self, width, height, devices):
        self._h = None
        L = _lib.load()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        _lib.check(L.vr_sharded_create(C.byref(h), devs, len(devices), int(width), int(height)))
        self._h, self._L = h, L
        self.devices = [int(d) for d in devices]
        self.parts = [Renderer(width, height, _borrowed=L.vr_sharded_part(h, i)) for i in range(L.vr_sharded_parts(h))]

    def close(self):
        if self._h is not None:
            for p in self.parts:
                p.close()
            self._L.vr_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def each(self, fn):
        """fn(part) for every part: how scene calls are replicated."""
        for p in self.parts:
            fn(p)
        return self

    @property
    def transport(self):
        return self._L.vr_sharded_transport(self._h).decode()

    @property
    def collective(self):
        """What the rccl transport runs per frame: "gather" (ncclSend / ncclRecv to part 0) or "allgather" (VR_SHARDED_COLLECTIVE)."""
        return self._L.vr_sharded_collective(self._h).decode()

    def reset(self):
        _lib.check(self._L.vr_sharded_reset(self._h))

    def render(self, spp=0, sync=True):
        _lib.check(self._L.vr_sharded_render(self._h, int(spp)))
        if sync:
            self.synchronize()

    def synchronize(self):
        _lib.check(self._L.vr_sharded_synchronize(self._h))

    def framebuffer(self):
        return self.parts[0].framebuffer()

    def save(self, path):
        self.parts[0].save(path)

    # ---- denoiser: every part computes the guides of its own tiles, part 0 gathers them and filters the whole frame ----
    def render_features(self, spp, sync=True):
        """Renderer.render_features on every part that owns tiles, over its tiles (vr_sharded_render_features); no exchange."""
        _lib.check(self._L.vr_sharded_render_features(self._h, int(spp)))
        if sync:
            self.synchronize()

    def render_features_expected(self, rays=2, sync=True):
        """Renderer.render_features_expected on every part that owns tiles, over its tiles (vr_sharded_render_features_expected); no exchange."""
        _lib.check(self._L.vr_sharded_render_features_expected(self._h, int(rays)))
        if sync:
            self.synchronize()

    expected_skip = _part0("expected_skip", True,
        """Whether the parts' expected-value passes drop the steps of empty space (Renderer.expected_skip): part 0's field; setting it sets every part's.
        Every part builds the clear-distance table of its own copy of the grid.""")
    expected_field = _part0("expected_field", True,
        """The field the parts' expected-value passes march (Renderer.expected_field: 0 trilinear, 1 the tracker's): part 0's field; setting it sets every part's.""")

    def gather_guides(self):
        """Every part's moments and features of its tiles into `parts[0]` (vr_sharded_gather_guides): one exchange, asynchronous."""
        _lib.check(self._L.vr_sharded_gather_guides(self._h))

    def denoise(self, sync=True):
        """gather_guides(), then Renderer.denoise's filter on `parts[0]` over the whole frame, with that part's `denoise_*` settings
        (vr_sharded_denoise): bit for bit the single-device result.  Needs `variance = 1` on every part for all the frame's samples."""
        _lib.check(self._L.vr_sharded_denoise(self._h))
        if sync:
            self.synchronize()

    def denoise_temporal(self, sync=True):
        """The same with Renderer.denoise_temporal's blend in front (vr_sharded_denoise_temporal); the history lives in `parts[0]`."""
        _lib.check(self._L.vr_sharded_denoise_temporal(self._h))
        if sync:
            self.synchronize()

    def denoised(self):
        return self.parts[0].denoised()

    def features(self):
        """[H][W][8] of the whole frame: gathers first."""
        self.gather_guides()
        return self.parts[0].features()

    def variance(self):
        """[H][W][4] of the whole frame: gathers first."""
        self.gather_guides()
        return self.parts[0].variance()

    def denoise_history(self):
        return self.parts[0].denoise_history()

    def denoise_history_reset(self):
        self.parts[0].denoise_history_reset()

    denoise_reject = _part0("denoise_reject", False,
        """The rejection threshold the filter runs with: part 0's (set it on `parts[0]`, or on every part with `each`).""")

    def denoise_reject_stat(self):
        return self.parts[0].denoise_reject_stat()

    denoise_moments = _part0("denoise_moments", False,
        """Whether the filter takes its variance from the history's luminance moments: part 0's field (set it on `parts[0]`, or on every part with `each`).""")

    def denoise_history_moments(self):
        return self.parts[0].denoise_history_moments()

    denoise_resolve = _part0("denoise_resolve", True,
        """Whether denoise() / denoise_temporal() start from the frame resolved against the expected coverage (Renderer.resolve): part 0's field, which
        holds the gathered frame and guide and runs the resolve; setting it sets every part's.""")

    denoise_layers = _part0("denoise_layers", True,
        """Whether denoise() / denoise_temporal() filter the scattered layer alone and put the analytic background back (Renderer.denoise_layers): part 0's
        field, which holds the gathered frame and guide and runs it; setting it sets every part's.""")

    denoise_filter = _part0("denoise_filter", True,
        """Whether one pass of local regression takes the place of the a-trous iterations (Renderer.denoise, csrc/vr_regress.h): part 0's field, which holds
        the gathered frame and guide and runs the filter; setting it sets every part's.""")

    denoise_demodulate = _part0("denoise_demodulate", True,
        """Whether the scattered layer is filtered divided by the guide's albedo (Renderer.denoise, csrc/vr_demod.h): part 0's field, which holds the
        gathered frame and guide and runs the filter; setting it sets every part's.""")

    denoise_ridge = _part0("denoise_ridge", True,
        """The ridge of that regression, 0 (zero order) or in [2^-20, 2^20]: part 0's field; setting it sets every part's.""")

    def denoised_layer(self):
        return self.parts[0].denoised_layer()


def math_probe(fn, a, b=None):
    a = _f32(a).reshape(-1)
    b = _f32(b).reshape(-1) if b is not None else np.zeros_like(a)
    out = np.empty_like(a)
    _lib.check(_lib.load().vr_math_probe(int(fn), a.ctypes.data, b.ctypes.data, out.ctypes.data, a.size))
    return out


def math_sweep(fn, first, count, b=0.0, out=None):
    """f(bits(first + i), b) for i < count (at most 2^26) on the device: float32 results, integer ones as their bit pattern."""
    if out is None:
        out = np.empty(int(count), np.float32)
    assert out.dtype == np.float32 and out.size >= count and out.flags.c_contiguous
    _lib.check(_lib.load().vr_math_sweep(int(fn), int(first) & 0xFFFFFFFF, int(count), float(b), out.ctypes.data))
    return out[:int(count)]


STATE_NAMES = ("new", "begin", "march", "collide", "nee", "postnee", "escape")
