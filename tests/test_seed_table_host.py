"""CPU: the path-seed table's index (vr_tiles.h seed_table_index) and its fill expression (vr_trace.h path_seed), built for the host, against TEA and the
tile layout written out here."""
import numpy as np
import pytest

import hk_seed as hs
import hk_tiles as ht

FRAMES = ((16, 16), (72, 56), (17, 1))      # exactly one tile; ragged on both axes, 5 x 4 tiles; one ragged row
M = 0xFFFFFFFF


def tea32(v0, v1):
    """common.glsl:40-52 in uint32 arithmetic: 32 rounds, returns v0"""
    s0 = 0
    for _ in range(32):
        s0 = (s0 + 0x9E3779B9) & M
        v0 = (v0 + ((((v1 << 4) & M) + 0xA341316C) & M ^ ((v1 + s0) & M) ^ (((v1 >> 5) + 0xC8013EA4) & M))) & M
        v1 = (v1 + ((((v0 << 4) & M) + 0xAD90777D) & M ^ ((v0 + s0) & M) ^ (((v0 >> 5) + 0x7E95761E) & M))) & M
    return v0


def want_seed(seed, w, px, py, smp):
    """do_new: tea32(seed * (py * W + px), smp), the product wrapping modulo 2^32"""
    return tea32(((seed & M) * ((py * w + px) & M)) & M, smp & M)


def test_pixel_zero_hashes_zero():
    """pixel 0 of any frame: the product is 0 whatever the seed, and the sample number alone separates its samples"""
    assert hs.path_seed(42, 64, 0, 0, 3) == tea32(0, 3) == hs.path_seed(7, 1031, 0, 0, 3)
    assert tea32(0, 3) != tea32(0, 4) and tea32(1, 2) != tea32(2, 1)


@pytest.mark.parametrize("seed", (42, 1, 0x7FFFFFFF, -5))
def test_path_seed_is_tea_of_the_wrapped_product(seed):
    w = 1031
    for px, py, smp in ((0, 0, 1), (1, 0, 1), (1030, 777, 1024), (5, 4_000_000, 7), (17, 33, 2 ** 31 - 1)):      # the fourth wraps py * W + px times seed
        assert hs.path_seed(seed, w, px, py, smp) == want_seed(seed, w, px, py, smp), (seed, px, py, smp)


@pytest.mark.parametrize("w,h", FRAMES)
def test_index_is_a_bijection_onto_its_range(w, h):
    n_tiles = ht.grid(w, h)[2]
    n_s = 3
    s, t, b, l = np.meshgrid(np.arange(n_s), np.arange(n_tiles), np.arange(4), np.arange(64), indexing="ij")
    i64, i32 = hs.index(s, n_tiles, t, b, l)
    assert np.array_equal(i64, i32.astype(np.uint64))
    assert np.array_equal(np.sort(i64.reshape(-1)), np.arange(n_s * n_tiles * 256, dtype=np.uint64))
    # the formula, and what it promises a NEW batch: a sub-tile's 64 lanes are adjacent, a sample's entries are one block
    assert np.array_equal(i64, (((s * n_tiles + t) * 4 + b) * 64 + l).astype(np.uint64))
    assert int(i64[1].min()) == n_tiles * 256 and int(i64[0].max()) == n_tiles * 256 - 1


@pytest.mark.parametrize("w,h", FRAMES)
def test_index_agrees_with_wave_tiled_pixel(w, h):
    """entry (s, tile, sub, lane) belongs to the pixel wave_tiled_pixel gives thread sub * 64 + lane of that tile -- the pixel make_unit and do_new give
    item lane of a unit of that sub-tile -- and tile_of_pixel / sub_of_pixel take the pixel back to it"""
    n_tiles = ht.grid(w, h)[2]
    seen = set()
    for tile in range(n_tiles):
        q = ht.pixels(tile, w)
        for t in range(256):
            _, sub, lane, px, py = (int(v) for v in q[t])
            assert ht.tile_of_pixel(px, py, w) == tile and hs.sub_of_pixel(px, py) == sub
            assert (px & 7) | ((py & 7) << 3) == lane                  # do_new: px = px0 + (item & 7), py = py0 + ((item >> 3) & 7)
            seen.add((px, py))
    assert len(seen) == n_tiles * 256
    assert all((x, y) in seen for x in range(w) for y in range(h))


@pytest.mark.parametrize("w,h", FRAMES)
def test_fill_holds_every_pixels_hash(w, h):
    seed, a, b = 42, 2, 5                                              # sample numbers 2..4 = the reference's samples 3..5
    n_tiles = ht.grid(w, h)[2]
    tab = hs.fill(seed, w, h, a, b)
    rng = np.random.default_rng(7)
    pix = {(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1)} | {(int(rng.integers(w)), int(rng.integers(h))) for _ in range(40)}
    for px, py in sorted(pix):
        tile, sub, lane = ht.tile_of_pixel(px, py, w), hs.sub_of_pixel(px, py), (px & 7) | ((py & 7) << 3)
        for s in range(a, b):
            i = int(hs.index(s - a, n_tiles, tile, sub, lane)[0])
            assert int(tab[i]) == want_seed(seed, w, px, py, s + 1), (px, py, s)
    # a fill of [a, b) is the tail of a fill of [0, b): the renderer fills the uncovered part of a launch's range only
    assert np.array_equal(hs.fill(seed, w, h, 0, b)[a * n_tiles * 256:], tab)
