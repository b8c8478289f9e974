// tests/hostkernel/seed_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The path-seed table's two definitions compiled for the host: where an entry lies (volren_amd/csrc/vr_tiles.h seed_table_index, in both index widths the
// product uses) and what it holds (volren_amd/csrc/vr_trace.h path_seed, the expression do_new and seed_fill_kernel share).  tests/test_seed_table_host.py
// checks both against statements of its own (tests/hk_seed.py).
#include <cstddef>
#include <cstdint>

#include "../../volren_amd/csrc/vr_tiles.h"
#include "../../volren_amd/csrc/vr_trace.h"

using namespace vr;

extern "C" {

// seed_table_index of n argument tuples: size_t (seed_fill_kernel) and uint32_t (the path-tracing kernel)
void hk_seed_index(int n, const uint32_t* s, int n_frame_tiles, const uint32_t* tile, const uint32_t* sub, const uint32_t* lane, uint64_t* out64, uint32_t* out32) {
    for (int i = 0; i < n; ++i) {
        out64[i] = (uint64_t)seed_table_index<size_t>((size_t)s[i], n_frame_tiles, (size_t)tile[i], sub[i], lane[i]);
        out32[i] = seed_table_index<uint32_t>(s[i], n_frame_tiles, tile[i], sub[i], lane[i]);
    }
}

// what seed_fill_kernel writes for the 0-based sample numbers [a, b) of a W x H frame: out[seed_table_index(s - a, ...)] for every thread of every tile
void hk_seed_fill(uint32_t seed, int W, int H, int a, int b, uint32_t* out) {
    const int32_t n_tiles = tile_count(W, H);
    for (int s = a; s < b; ++s)
        for (int32_t tile = 0; tile < n_tiles; ++tile)
            for (uint32_t t = 0; t < 256u; ++t) {
                const TilePixel q = wave_tiled_pixel(tile, t, W);
                out[seed_table_index<size_t>((size_t)(s - a), n_tiles, (size_t)tile, (uint32_t)q.sub, (uint32_t)q.lane)] = path_seed(seed, W, q.px, q.py, s + 1);
            }
}

uint32_t hk_seed_path(uint32_t seed, int W, int px, int py, int smp) { return path_seed(seed, W, px, py, smp); }
uint32_t hk_seed_sub_of_pixel(int px, int py) { return sub_of_pixel(px, py); }

}
