"""CPU: the wire format of the sharded renderer's packed denoiser guides (vr_tiles.h guide_slot with raster_in_tile_pixel, built for the host) in a
numpy model of pack_guides_kernel -> the exchange (buffers concatenated in part order) -> unpack_guides_kernel, over the product's own tile deal."""
import numpy as np
import pytest

import hk_guides as hg
import volren_amd

FRAMES = ((16, 16), (32, 32), (70, 52), (150, 90))
PARTS = (1, 2, 3, 5, 8)


def _owner_lists(w, h, n_parts):
    """tile_owner_lists of sharded.cpp through the C ABI (host only)"""
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    owners = np.zeros(n_tiles, np.int32)
    assert volren_amd.load().vr_tile_owners(w, h, n_parts, owners.ctypes.data, n_tiles) == 0
    return [[int(t) for t in np.nonzero(owners == p)[0]] for p in range(n_parts)]


def test_the_index_is_the_stated_expression_and_dense():
    assert hg.planes() == 3
    s = hg.slots(0, 7)
    k, p, t = np.meshgrid(np.arange(7), np.arange(3), np.arange(256), indexing="ij")
    assert np.array_equal(s, ((k * 3 + p) * 256 + t).astype(np.uint64))
    assert np.array_equal(np.sort(s.reshape(-1)), np.arange(7 * 3 * 256, dtype=np.uint64))       # a part's buffer is one contiguous run
    big = hg.slots((1 << 31) // 256, 1)                                                          # no 32-bit wrap in the index itself
    assert int(big[0, 2, 255]) == (((1 << 31) // 256) * 3 + 2) * 256 + 255


@pytest.mark.parametrize("n_parts", PARTS)
@pytest.mark.parametrize("w,h", FRAMES)
def test_pack_exchange_unpack_round_trip(w, h, n_parts):
    rs = np.random.RandomState(w * 1000 + h * 10 + n_parts)
    moments = rs.uniform(-1, 1, (h, w, 4)).astype(np.float32)
    features = rs.uniform(-1, 1, (h, w, 8)).astype(np.float32)
    lists = _owner_lists(w, h, n_parts)
    assert sorted(t for l in lists for t in l) == list(range(((w + 15) // 16) * ((h + 15) // 16)))
    n_max = max(1, max(len(l) for l in lists))
    per_part = n_max * 3 * 256                                # float4 a part contributes
    slot_index = hg.slots(0, n_max).astype(np.int64)          # [n_max][3][256]
    assert int(slot_index.max()) < per_part
    # pack (sharded.cpp setup: the list is padded by repeating the last tile; a part without tiles packs nothing and sends zeros)
    gathered = np.zeros((n_parts * per_part, 4), np.float32)
    padding = np.zeros(n_parts * per_part, bool)              # float4 of padding slots: unpack must not read them
    unpack_ids = []
    for p, own in enumerate(lists):
        packed = np.full((per_part, 4), np.nan, np.float32) if own else np.zeros((per_part, 4), np.float32)
        pack_ids = own + [own[-1] if own else 0] * (n_max - len(own))
        for k, tile in enumerate(pack_ids if own else []):
            q = hg.pixels(tile, w)
            inside = (q[:, 0] < w) & (q[:, 1] < h)
            for plane in range(3):
                v = np.zeros((256, 4), np.float32)            # outside the frame: zeros
                src = moments if plane == 0 else features[..., 4 * (plane - 1):4 * plane]
                v[inside] = src[q[inside, 1], q[inside, 0]]
                packed[slot_index[k, plane]] = v
        assert not np.isnan(packed).any()                     # every float4 of the part's buffer was written
        gathered[p * per_part:(p + 1) * per_part] = packed
        padding[p * per_part + len(own) * 3 * 256:(p + 1) * per_part] = True
        unpack_ids += own + [-1] * (n_max - len(own))
    assert len(unpack_ids) == n_parts * n_max
    gathered[padding] = np.nan                                # poison: a read of a padding slot would show
    # unpack: one workgroup per slot of the gathered buffer, in part order
    all_index = hg.slots(0, n_parts * n_max).astype(np.int64)
    assert int(all_index.max()) < n_parts * n_max * 3 * 256 == gathered.shape[0]
    out_m = np.full((h, w, 4), np.nan, np.float32)
    out_f = np.full((h, w, 8), np.nan, np.float32)
    writes = np.zeros((h, w, 3), np.int32)
    read = np.zeros(gathered.shape[0], bool)
    for slot, tile in enumerate(unpack_ids):
        if tile < 0:
            continue
        q = hg.pixels(tile, w)
        inside = (q[:, 0] < w) & (q[:, 1] < h)
        for plane in range(3):
            idx = all_index[slot, plane][inside]
            read[idx] = True
            dst = out_m if plane == 0 else out_f[..., 4 * (plane - 1):4 * plane]
            dst[q[inside, 1], q[inside, 0]] = gathered[idx]
            np.add.at(writes[..., plane], (q[inside, 1], q[inside, 0]), 1)
    assert (writes == 1).all()                                # every pixel of the frame exactly once, each of its three float4
    assert not (read & padding).any()
    assert np.array_equal(out_m.view(np.uint32), moments.view(np.uint32))
    assert np.array_equal(out_f.view(np.uint32), features.view(np.uint32))
