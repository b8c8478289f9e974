// tests/hostkernel/tiles_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The tile layout of the product (volren_amd/csrc/vr_tiles.h) compiled for the host: tests/test_tiles_host.py checks both thread layouts, the
// staged window of a tile (TileWindow), the sample pool's slots and the variance factor against statements of its own (tests/hk_tiles.py).
#include <cstddef>
#include <cstdint>

#include "../../volren_amd/csrc/vr_tiles.h"

using namespace vr;

extern "C" {

void hk_tiles_grid(int W, int H, int32_t* out) { out[0] = tiles_x(W); out[1] = tiles_y(H); out[2] = tile_count(W, H); }
int hk_tiles_of_pixel(int px, int py, int W) { return tile_of_pixel(px, py, W); }

// every thread 0..255 of the workgroup that serves `tile`: out[t] = (tile, sub, lane, px, py); raster = 0: wave-tiled, 1: raster in the tile
void hk_tiles_pixels(int raster, int tile, int W, int32_t* out) {
    for (uint32_t t = 0; t < 256u; ++t) {
        const TilePixel q = raster ? raster_in_tile_pixel(tile, t, W) : wave_tiled_pixel(tile, t, W);
        int32_t* o = out + 5 * t;
        o[0] = q.tile; o[1] = q.sub; o[2] = q.lane; o[3] = q.px; o[4] = q.py;
    }
}

// pool_slot of n argument tuples, in both index widths the product uses (size_t: the accumulate kernel, uint32_t: make_unit)
void hk_tiles_pool_slots(int n, const uint32_t* chunk, int n_tiles, const uint32_t* tile_slot, const uint32_t* sub, int spu, const uint32_t* sample,
                         const uint32_t* lane, uint64_t* out64, uint32_t* out32) {
    for (int i = 0; i < n; ++i) {
        out64[i] = (uint64_t)pool_slot<size_t>((size_t)chunk[i], n_tiles, (size_t)tile_slot[i], sub[i], spu, (size_t)sample[i], lane[i]);
        out32[i] = pool_slot<uint32_t>(chunk[i], n_tiles, tile_slot[i], sub[i], spu, sample[i], lane[i]);
    }
}

float hk_tiles_variance_scale(int n) { return variance_scale(n); }

// TileWindow<R> of `tile`, R = 2 or 3 (the halos the staged kernels use): geom = (kFoot, kTexels, x0, y0), at[t] = at(px, py) of the wave-tiled thread t's
// pixel.  -> 0, or -1 for another R
int hk_tiles_window(int R, int tile, int W, int32_t* geom, int32_t* at) {
    const auto fill = [&](auto window) {
        geom[0] = window.kFoot; geom[1] = window.kTexels; geom[2] = window.x0; geom[3] = window.y0;
        for (uint32_t t = 0; t < 256u; ++t) {
            const TilePixel q = wave_tiled_pixel(tile, t, W);
            at[t] = window.at(q.px, q.py);
        }
        return 0;
    };
    if (R == 2) return fill(TileWindow<2>::of(tile, W));
    if (R == 3) return fill(TileWindow<3>::of(tile, W));
    return -1;
}

}
