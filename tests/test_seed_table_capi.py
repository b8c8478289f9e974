"""CPU: the C ABI of the path-seed table -- the settings "seed_table_mb" / "seed_table_max_samples", the read-only "seed_table_samples" /
"seed_table_fills", and the two host-only functions that state the table's arithmetic -- exported, listed, documented with their ranges and defaults.
A renderer needs a device: where one is present the values are checked here too, and tests/test_gpu_seed_table.py checks them in any case."""
import os

import scenes
import volren_amd
from test_capi_symbols import declared_functions

NEW = ("vr_seed_table_default_mb", "vr_seed_table_samples_for")


def test_the_new_symbols_are_exported_listed_and_documented():
    lib = volren_amd.load()
    for name in NEW:
        assert hasattr(lib, name) and name in volren_amd.SYMBOLS and name in declared_functions(), name
    text = open(os.path.join(scenes.ROOT, "include", "volren_amd.h")).read()
    for word in ('"seed_table_mb"', '"seed_table_max_samples"', '"seed_table_samples"', '"seed_table_fills"', "0 .. 8192", 'min(4096, "sample_pool_mb" / 4)',
                 "vr_reset keeps it", "no render fails for it", "Results never depend on the table"):
        assert word in text, word


def test_the_default_follows_the_sample_pool():
    lib = volren_amd.load()
    f = lib.vr_seed_table_default_mb
    assert f(65536) == 4096                             # the renderer's default pool: 4 GiB, a 1024^2 frame of 1024 spp in full
    assert f(16384) == 4096 and f(16383) == 4095        # the point where the pool starts to limit it
    assert f(64) == 16 and f(16) == 4                   # renderers whose pool a test made small stay small
    assert f(3) == 0 and f(0) == 0 and f(-1) == 0


def test_samples_a_budget_covers():
    lib = volren_amd.load()
    g = lib.vr_seed_table_samples_for
    assert g(4096, 1024, 1024) == 1024                  # 4 bytes x 2^20 pixels per sample
    assert g(4096, 2048, 2048) == 256
    assert g(1, 72, 56) == (1 << 20) // (20 * 256 * 4)  # a ragged frame pays for its 5 x 4 whole tiles
    assert g(1, 17, 1) == (1 << 20) // (2 * 256 * 4)
    assert g(0, 64, 64) == 0 and g(-1, 64, 64) == 0 and g(16, 0, 64) == 0 and g(16, 64, -3) == 0
    assert g(8192, 1, 1) == 8192 * 1024                 # the largest budget on the smallest frame: far inside an int


def check_values(r):
    """the settings on renderer r: ranges, defaults, and what the read-only names say before any launch"""
    lib = volren_amd.load()
    assert r.sample_pool_mb == 65536 and r.seed_table_mb == 4096 and r.seed_table_max_samples == 0
    assert r.seed_table_samples == 0 and r.seed_table_fills == 0
    r.sample_pool_mb = 64
    assert r.seed_table_mb == 16                        # the default follows the pool ...
    r.seed_table_mb = 7
    r.sample_pool_mb = 4096
    assert r.seed_table_mb == 7                         # ... a value that was set does not
    r.seed_table_mb = -1
    assert r.seed_table_mb == 1024                      # -1: back to the default
    for v in (0, 1, 8192):
        r.seed_table_mb = v
        assert r.seed_table_mb == v and r.get_int("seed_table_mb") == v
        for bad in (-2, 8193, 2 ** 31 - 1):
            assert lib.vr_set_int(r._h, b"seed_table_mb", bad) == 1 and b"seed_table_mb" in lib.vr_last_error()
            assert r.seed_table_mb == v
    r.seed_table_max_samples = 12
    assert r.seed_table_max_samples == 12
    assert lib.vr_set_int(r._h, b"seed_table_max_samples", -1) == 1 and r.seed_table_max_samples == 12
    for name in (b"seed_table_samples", b"seed_table_fills"):
        assert lib.vr_set_int(r._h, name, 1) == 1 and b"unknown int parameter" in lib.vr_last_error()      # read-only


def test_the_values_where_a_renderer_can_exist():
    if volren_amd.load().vr_device_count() > 0:
        check_values(volren_amd.Renderer(16, 16))


def test_the_python_layer_carries_the_new_names():
    from volren_amd import renderer
    assert "seed_table_mb" in renderer._INT_FIELDS and "seed_table_max_samples" in renderer._INT_FIELDS
    src = open(renderer.__file__).read()
    assert '"seed_table_samples"' in src and '"seed_table_fills"' in src
