"""CPU: the tile layout every per-pixel kernel, make_unit and the host share (vr_tiles.h), built for the host, against statements written here."""
import numpy as np
import pytest

import hk_tiles as ht

FRAMES = ((1, 1), (16, 16), (17, 9), (40, 24))      # smallest; exactly one tile; ragged on both axes; ragged with several tiles


def _grid(w, h):
    return (w + 15) // 16, (h + 15) // 16


@pytest.mark.parametrize("w,h", FRAMES)
def test_tile_grid(w, h):
    tx, ty = _grid(w, h)
    assert ht.grid(w, h) == (tx, ty, tx * ty)
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2)):
        assert ht.tile_of_pixel(x, y, w) == (y // 16) * tx + x // 16


@pytest.mark.parametrize("raster", (False, True), ids=("wave_tiled", "raster_in_tile"))
@pytest.mark.parametrize("w,h", FRAMES)
def test_every_pixel_once_and_inside_its_tile(w, h, raster):
    tx, ty = _grid(w, h)
    hits = np.zeros((h, w), np.int32)
    for tile in range(tx * ty):
        q = ht.pixels(tile, w, raster)
        x0, y0 = (tile % tx) * 16, (tile // tx) * 16
        assert (q[:, 0] == tile).all()
        assert (q[:, 3] >= x0).all() and (q[:, 3] < x0 + 16).all() and (q[:, 4] >= y0).all() and (q[:, 4] < y0 + 16).all()
        assert len({(int(a), int(b)) for a, b in q[:, 3:5]}) == 256          # the 256 threads cover the tile's square
        inside = (q[:, 3] < w) & (q[:, 4] < h)
        np.add.at(hits, (q[inside, 4], q[inside, 3]), 1)
    assert (hits == 1).all()


@pytest.mark.parametrize("w,h", FRAMES)
def test_layouts_thread_by_thread(w, h):
    tx, ty = _grid(w, h)
    t = np.arange(256)
    for tile in range(tx * ty):
        x0, y0 = (tile % tx) * 16, (tile // tx) * 16
        q = ht.pixels(tile, w)
        sub, lane = t >> 6, t & 63
        assert np.array_equal(q[:, 1], sub) and np.array_equal(q[:, 2], lane)
        # make_unit takes a unit's (px0, py0) from lane 0 of the sub-tile, and the path tracer puts item i of the unit at
        # (px0 + (i & 7), py0 + ((i >> 3) & 7)): both must be the wave-tiled pixel of thread sub * 64 + (i & 63)
        for s in range(4):
            px0, py0 = q[s * 64, 3], q[s * 64, 4]
            assert (px0, py0) == (x0 + 8 * (s & 1), y0 + 8 * (s >> 1))
            item = np.arange(512)                             # 8 samples of the unit: the pixel does not depend on the sample
            assert np.array_equal(q[s * 64 + (item & 63), 3], px0 + (item & 7)) and np.array_equal(q[s * 64 + (item & 63), 4], py0 + ((item >> 3) & 7))
        r = ht.pixels(tile, w, raster=True)
        assert np.array_equal(r[:, 3], x0 + (t & 15)) and np.array_equal(r[:, 4], y0 + (t >> 4))
        assert (r[:, 1] == 0).all() and (r[:, 2] == 0).all()


@pytest.mark.parametrize("spu", (8, 4))
@pytest.mark.parametrize("w,h", FRAMES)
def test_pool_slots_are_distinct_and_dense(w, h, spu):
    n_samples = 11                                            # the last chunk is partial: 3 of 8, 3 of 4
    n_all = ht.grid(w, h)[2]
    subset = [0, 2, 5] if n_all >= 6 else list(range(n_all))
    chunks = (n_samples + spu - 1) // spu
    for n_tiles in sorted({3, len(subset)}):                  # a 3-tile list (the slots know the list's length only), and the frame's own
        total = chunks * n_tiles * 4 * spu * 64
        c, s, b, k, l = np.meshgrid(np.arange(chunks), np.arange(n_tiles), np.arange(4), np.arange(spu), np.arange(64), indexing="ij")
        s64, s32 = ht.pool_slots(c, n_tiles, s, b, spu, k, l)
        assert np.array_equal(s64, s32.astype(np.uint64))
        assert np.array_equal(np.sort(s64.reshape(-1)), np.arange(total, dtype=np.uint64))
        # a unit's items are contiguous from its base (WorkUnit::base + item, item = sample-in-chunk * 64 + lane), units in the order
        # u = (chunk * n_tiles + slot) * 4 + sub-tile
        base = s64[:, :, :, 0, 0]
        assert np.array_equal(s64, base[..., None, None] + (k * 64 + l).astype(np.uint64))
        assert np.array_equal(base, (((c * n_tiles + s) * 4 + b) * spu * 64)[:, :, :, 0, 0].astype(np.uint64))
        # what the accumulate kernel reads for samples 0..10: chunk = k / spu, sample-in-chunk = k - chunk * spu
        kk = np.arange(n_samples)
        used, _ = ht.pool_slots((kk // spu)[:, None, None, None], n_tiles, np.arange(n_tiles)[None, :, None, None], np.arange(4)[None, None, :, None],
                                spu, (kk % spu)[:, None, None, None], np.arange(64)[None, None, None, :])
        assert np.unique(used).size == n_samples * n_tiles * 256 and int(used.max()) < total
    # with the subset list, slot (tile slot, sub, lane) is the pixel of thread sub * 64 + lane of tile subset[tile slot]: distinct pixels
    seen = set()
    for tile in subset:
        q = ht.pixels(tile, w)
        seen |= {(int(a), int(b)) for a, b in q[:, 3:5]}
    assert len(seen) == 256 * len(subset)


# thin both ways, one past a tile on either axis, one short of two tiles, several ragged tiles: the halo leaves the frame on every side in turn
WINDOW_FRAMES = ((1, 1), (1, 37), (37, 1), (17, 16), (33, 31), (40, 24))


@pytest.mark.parametrize("r", (2, 3))
@pytest.mark.parametrize("w,h", WINDOW_FRAMES)
def test_staged_window_holds_every_neighbour_where_the_kernels_look(w, h, r):
    """TileWindow<R>: texel f of the footprint is the frame coordinate (x0 + f % kFoot, y0 + f / kFoot) -- how stage_window fills it -- and a thread finds
    its neighbour (dx, dy) at at(px, py) + dy * kFoot + dx -- how the *WindowDev accessors read it."""
    tx, ty = _grid(w, h)
    d = np.arange(-r, r + 1)
    dx, dy = np.meshgrid(d, d, indexing="xy")
    for tile in range(tx * ty):
        (foot, texels, x0, y0), at = ht.window(r, tile, w)
        assert (foot, texels) == (16 + 2 * r, (16 + 2 * r) ** 2)
        f = np.arange(texels)
        fx, fy = x0 + f % foot, y0 + f // foot
        # one-to-one onto the tile's square grown by r on every side
        tx0, ty0 = (tile % tx) * 16, (tile // tx) * 16
        want = {(x, y) for x in range(tx0 - r, tx0 + 16 + r) for y in range(ty0 - r, ty0 + 16 + r)}
        assert len(want) == texels and set(zip(fx.tolist(), fy.tolist())) == want
        q = ht.pixels(tile, w)
        inside = (q[:, 3] < w) & (q[:, 4] < h)
        assert inside.any()
        px, py, a = q[inside, 3], q[inside, 4], at[inside]
        idx = a[:, None, None] + dy[None] * foot + dx[None]
        assert idx.min() >= 0 and idx.max() < texels
        assert np.array_equal(fx[idx], px[:, None, None] + dx[None]) and np.array_equal(fy[idx], py[:, None, None] + dy[None])


def test_variance_scale_is_the_literal_expression():
    for n in (0, 1, 2, 3, 16777217):
        want = np.float32(n) / np.float32(n - 1) if n >= 2 else np.float32(0.0)
        assert ht.variance_scale(n).view(np.uint32) == np.float32(want).view(np.uint32), n
    assert np.float32(16777217) == np.float32(16777216)       # (float)n rounds: n / (n - 1) is 1 there, as in the product
    assert ht.variance_scale(16777217) == np.float32(1.0)
