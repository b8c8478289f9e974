"""CPU: the two addressing forms of the path-tracing kernels' gathers (vr_trace.h table_load / line_load) read the same elements, and the rule that chooses
between them per launch (vr_scene.h grid_largest_table_bytes, vr_variant.h pathtrace_kernel_of: 64-bit addresses from 4 GiB on) says what the layouts of
DESIGN.md 4 say, at the extents where the answer changes -- which no GPU test can afford to build."""
import hk_hotpair as hp

GIB4 = 1 << 32


def test_both_forms_read_the_same_elements():
    # 37 bricks / dense blocks (odd, several 128-byte lines of every kind) and a majorant table that is no multiple of a line
    assert hp.addressing_forms_differ(37, 1000) == 0


def _mshift(nb):
    return tuple(max(3, (max(n, 1) - 1).bit_length()) for n in nb)


def test_brick_atlas_threshold():
    # 640 bytes per brick of the grid's box: 4 GiB at 6710886.4 bricks
    for nb, wide in (((189, 189, 187), False), ((189, 189, 188), True), ((128, 128, 128), False), ((256, 256, 128), True)):
        b = hp.largest_table_bytes(nb=nb, mshift=_mshift(nb))
        assert b == nb[0] * nb[1] * nb[2] * 640
        assert (b >= GIB4) == wide, nb


def test_paired_and_float_atlas_thresholds():
    nb = (128, 128, 128)                                   # 2^21 bricks: 1.25 GiB of blocks, 2.5 GiB paired, exactly 4 GiB decoded to floats
    ms = _mshift(nb)
    assert hp.largest_table_bytes(nb=nb, mshift=ms, paired=True) == (1 << 21) * 1280 < GIB4
    assert hp.largest_table_bytes(nb=nb, mshift=ms, float_atlas=True, tf=True) == GIB4
    nb = (128, 128, 127)
    assert hp.largest_table_bytes(nb=nb, mshift=_mshift(nb), float_atlas=True, tf=True) == 128 * 128 * 127 * 2048 < GIB4


def test_dense_grid_threshold():
    # 4x4x4 blocks of 128 bytes: 2 bytes per voxel of the padded extent
    for dim, wide in (((1288, 1288, 1288), False), ((1292, 1292, 1292), True), ((2048, 2048, 508), False), ((2048, 2048, 512), True), ((1021, 1023, 1022), False)):
        ms = _mshift(tuple((d + 7) // 8 for d in dim))
        b = hp.largest_table_bytes(dim=dim, mshift=ms)
        assert b == ((dim[0] + 3) // 4) * ((dim[1] + 3) // 4) * ((dim[2] + 3) // 4) * 128
        assert (b >= GIB4) == wide, dim


def test_majorant_table_threshold():
    # 585/512 x 2^k + 1 cells (four levels and the "outside" cell): the fp16 table never reaches 4 GiB (k <= 30), the float table of a transfer-function render does at k = 30
    cells = lambda k: (585 << (k - 9)) + 1
    assert hp.largest_table_bytes(mshift=(10, 10, 10), tf=False) == cells(30) * 2 < GIB4
    assert hp.largest_table_bytes(mshift=(10, 10, 10), tf=True) == cells(30) * 4 >= GIB4
    assert hp.largest_table_bytes(mshift=(10, 10, 9), tf=True) == cells(29) * 4 < GIB4
