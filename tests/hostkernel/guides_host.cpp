// tests/hostkernel/guides_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The wire format of the sharded renderer's packed denoiser guides (volren_amd/csrc/vr_tiles.h guide_slot, with raster_in_tile_pixel) compiled for the
// host: tests/test_sharded_guides_host.py runs a pack -> concatenate -> unpack round trip over it in numpy (tests/hk_guides.py).
#include <cstddef>
#include <cstdint>

#include "../../volren_amd/csrc/vr_tiles.h"

using namespace vr;

extern "C" {

int hk_guides_planes() { return (int)kGuidePlanes; }

// float4 index of (tile slot, plane, thread) for every plane and thread of tile slots first .. first + n - 1: out[n][planes][256]
void hk_guides_slots(uint64_t first, int n, uint64_t* out) {
    for (int s = 0; s < n; ++s)
        for (uint32_t p = 0; p < kGuidePlanes; ++p)
            for (uint32_t t = 0; t < 256u; ++t) out[((size_t)s * kGuidePlanes + p) * 256u + t] = (uint64_t)guide_slot((size_t)(first + (uint64_t)s), p, t);
}

// the pixel of thread t of the workgroup that packs or unpacks `tile`: out[256][2] = (px, py)
void hk_guides_pixels(int tile, int W, int32_t* out) {
    for (uint32_t t = 0; t < 256u; ++t) {
        const TilePixel q = raster_in_tile_pixel(tile, t, W);
        out[2 * t] = q.px; out[2 * t + 1] = q.py;
    }
}

}
