"""ctypes loader for libvolren_amd.so (the C ABI declared in include/volren_amd.h).

The library is the product: hand-written HIP kernels for gfx950 plus the C++ host classes.  There is no
fallback -- if the shared object is missing, or no HIP device is visible when a compute entry point is called,
this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VOLREN_AMD_LIB") or os.path.join(_HERE, "libvolren_amd.so")      # override: tuning builds (tests/tools_build_variant.sh)

vp, ci, cf, cd, cs, ll = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_char_p, C.c_longlong


def _sig(argtypes, names, restype=ci):
    return {n: (argtypes, restype) for n in names.split()}


# Every symbol include/volren_amd.h declares (checked by tests/test_capi_symbols.py) with its (argtypes, restype), grouped by signature: a new function
# of a signature that is here already is one more name in that row.  argtypes None: the symbol gets none (it takes no argument, or one handle).
_SIGNATURES = {
    **_sig(None, "vr_last_error vr_version", cs),
    **_sig(None, "vr_device_count vr_uniforms_size vr_flush"),
    **_sig([vp], "vr_destroy vr_sharded_destroy", None),
    **_sig([vp], "vr_sharded_transport vr_sharded_collective", cs),
    **_sig([vp], "vr_commit vr_reset vr_scale_and_move_to_unit_cube vr_trace vr_synchronize vr_draw vr_denoise vr_denoise_temporal vr_denoise_history_reset "
                 "vr_resolve vr_impmap_floats vr_sharded_parts vr_sharded_reset vr_sharded_synchronize vr_sharded_gather_guides vr_sharded_denoise "
                 "vr_sharded_denoise_temporal"),
    **_sig([vp, ci], "vr_render vr_render_features vr_render_features_expected vr_sharded_render vr_sharded_render_features vr_sharded_render_features_expected"),
    **_sig([vp, ci], "vr_sharded_part", vp),
    **_sig([vp, ci, ci], "vr_resize vr_upsample"),
    # whole-frame read-backs and other (handle, pointer) calls
    **_sig([vp, vp], "vr_framebuffer vr_display vr_features vr_variance vr_denoised vr_denoise_reject_stat vr_denoise_history_moments vr_resolved "
                     "vr_resolve_background vr_denoised_layer vr_upsampled vr_upsampled_layer vr_upsampled_features vr_upsampled_size vr_expected_stats "
                     "vr_volume_n_grid_frames vr_set_stream vr_set_sched vr_grid_checksums"),
    **_sig([vp, vp, vp], "vr_expected_clear_table"),
    **_sig([vp, vp, vp, vp], "vr_denoise_history"),
    **_sig([vp, vp, ci], "vr_set_transferfunc vr_tile_samples vr_tile_error vr_set_tiles vr_get_uniforms vr_get_impmap vr_wave_timeline"),
    **_sig([vp, vp, ci, ci], "vr_set_envmap"),
    **_sig([vp, vp, ci, vp], "vr_pack_tiles vr_unpack_tiles"),
    **_sig([vp, ci, vp], "vr_sched_stats"),
    **_sig([vp, ci, ci, cf], "vr_render_adaptive"),
    **_sig([vp, C.POINTER(cd)], "vr_last_kernel_ms vr_last_pathtrace_ms"),
    **_sig([vp, C.POINTER(vp)], "vr_framebuffer_device"),
    **_sig([vp, cs], "vr_load_volume vr_set_volume_path vr_load_envmap vr_load_transferfunc vr_save_png"),
    **_sig([vp, cs, ci], "vr_set_int"),
    **_sig([vp, cs, C.POINTER(ci)], "vr_get_int"),
    **_sig([vp, cs, C.POINTER(cf)], "vr_volume_aabb vr_volume_minorant_majorant"),
    **_sig([vp, cs, C.POINTER(cf), ci], "vr_set_float vr_get_float"),
    **_sig([vp, cs, vp, ci, ci, ci, vp, ci], "vr_set_volume_dense vr_set_volume_dense_f16"),
    **_sig([vp, cs, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, ci], "vr_set_volume_brick"),
    **_sig([vp, cs, vp, ci, ci, ci, vp], "vr_volume_add_grid_frame_dense"),
    **_sig([vp, ci, cs, vp, ci, ci, ci, vp], "vr_volume_update_grid_frame_dense"),
    **_sig([C.POINTER(vp), ci, ci, ci], "vr_create"),
    **_sig([C.POINTER(vp), C.POINTER(ci), ci, ci, ci], "vr_sharded_create"),
    **_sig([ci], "vr_seed_table_default_mb"),
    **_sig([ci, ci, ci], "vr_seed_table_samples_for"),
    **_sig([ci, ci, ci, vp, ci], "vr_tile_owners"),
    **_sig([ll], "vr_test_alloc_cap_mb"),
    **_sig([ci, vp, vp, vp, ci], "vr_math_probe"),
    **_sig([ci, C.c_uint32, ll, cf, vp], "vr_math_sweep"),
    **_sig([vp, ci, ci, vp, vp, ll], "vr_probe vr_path_probe"),
    **_sig([vp, ci, ci, ci, vp, vp, vp], "vr_filter_probe"),
    **_sig([vp, ci, ci, ci, vp, cs], "vr_write_brick_from_dense"),
    **_sig([vp, ci, ci, ci, cf, cf, vp, cs], "vr_write_dense"),
    **_sig([vp, ci, ci, ci, vp, vp, vp], "vr_encode_dense_stats"),
}
SYMBOLS = list(_SIGNATURES)

_lib = None


class VolrenError(RuntimeError):
    pass


def load():
    """Load the library (torch first, so that both share one libamdhip64 when torch is used in the process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VolrenError("libvolren_amd.so is not built (%s). Run `make` or __graft_entry__.build(); there is no "
                          "CPU/PyTorch fallback for the HIP path." % LIB_PATH)
    try:  # noqa: SIM105 -- torch is optional plumbing (streams, torch.distributed); the renderer itself does not need it
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(L, name)
        if argtypes is not None:
            fn.argtypes = list(argtypes)
        fn.restype = restype
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise VolrenError(load().vr_last_error().decode("utf-8", "replace") or ("error code %d" % rc))
