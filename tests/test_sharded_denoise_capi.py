"""CPU: the C ABI of denoising on the sharded renderer (vr_sharded_render_features, vr_sharded_gather_guides, vr_sharded_denoise,
vr_sharded_denoise_temporal) -- exported, listed, declared, and refusing a NULL object."""
import volren_amd
import test_capi_symbols
from test_capi_symbols import declared_functions

NEW = ("vr_sharded_render_features", "vr_sharded_gather_guides", "vr_sharded_denoise", "vr_sharded_denoise_temporal")


def test_new_symbols_are_exported_listed_and_declared():
    lib = volren_amd.load()
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in volren_amd.SYMBOLS, n
        assert n in declared_functions(), n


def test_the_header_and_the_library_still_agree():
    test_capi_symbols.test_header_symbols_are_exported()


def test_null_object_is_rejected():
    lib = volren_amd.load()
    assert lib.vr_sharded_render_features(None, 2) == 3 and b"null sharded renderer" in lib.vr_last_error()      # VR_ERR_ARG
    for n in NEW[1:]:
        assert getattr(lib, n)(None) == 3, n
        assert b"null sharded renderer" in lib.vr_last_error()


def test_python_sharded_renderer_has_the_calls():
    for n in ("render_features", "gather_guides", "denoise", "denoise_temporal", "denoised", "features", "variance", "denoise_history",
              "denoise_history_reset"):
        assert callable(getattr(volren_amd.ShardedRenderer, n)), n
