// vr_tiles.h -- the one definition of how a frame is cut into tiles, and of what follows from it (host + device).
// A W x H frame (row 0 at the bottom) is cut into 16x16 tiles in raster order, tile = ty * tiles_x + tx.  A workgroup's 256 threads lie in a tile
//   wave-tiled : as four 8x8 sub-tiles, one per wavefront (sub-tile s at (8 (s & 1), 8 (s >> 1)), lane l at (l & 7, l >> 3) in it) -- every per-pixel
//                kernel, and the path tracer's work units (vr_pathtrace.h make_unit: a unit is one sub-tile x spu samples); or
//   raster     : thread t at (t & 15, t >> 4) -- the packed tiles of the sharded framebuffer and of its denoiser guides only, whose texel order is wire format.
// Also here: the window of a tile's pixels plus a halo that a kernel stages in LDS (TileWindow, stage_window), the same for a tile of a frame F times the staged
// one's size (ScaledTileWindow), and the wire and table indices below.
// tests/hostkernel/tiles_host.cpp and guides_host.cpp build this header for the host.
#pragma once

#include <stddef.h>

#include "vr_math.h"

namespace vr {

// tile grid of a W x H frame
VR_HD int32_t tiles_x(int32_t W) { return (W + 15) >> 4; }
VR_HD int32_t tiles_y(int32_t H) { return (H + 15) >> 4; }
VR_HD int32_t tile_count(int32_t W, int32_t H) { return tiles_x(W) * tiles_y(H); }
VR_HD int32_t tile_of_pixel(int32_t px, int32_t py, int32_t W) { return (py >> 4) * tiles_x(W) + (px >> 4); }

struct TilePixel {
    int32_t tile, sub, lane;      // raster tile id, 8x8 sub-tile 0..3, lane 0..63 in the sub-tile (wave-tiled layout only: sub = lane = 0 in the raster one)
    int32_t px, py;               // may lie outside a frame whose size is no multiple of 16: the caller tests px < W && py < H
};

// wave-tiled layout: thread t (0..255) of the workgroup that serves `tile`
VR_HD TilePixel wave_tiled_pixel(int32_t tile, uint32_t t, int32_t W) {
    const int32_t nx = tiles_x(W), sub = (int32_t)(t >> 6), lane = (int32_t)(t & 63u);
    return TilePixel{ tile, sub, lane, (tile % nx) * 16 + ((sub & 1) << 3) + (lane & 7), (tile / nx) * 16 + ((sub >> 1) << 3) + (lane >> 3) };
}
// the OTHER layout, raster in the tile -- pack_tiles_kernel / unpack_tiles_kernel only
VR_HD TilePixel raster_in_tile_pixel(int32_t tile, uint32_t t, int32_t W) {
    const int32_t nx = tiles_x(W);
    return TilePixel{ tile, 0, 0, (tile % nx) * 16 + (int32_t)(t & 15u), (tile / nx) * 16 + (int32_t)(t >> 4) };
}
// The window a workgroup stages for its tile: the tile's 16 x 16 pixels plus a halo of R on every side, kFoot x kFoot texels in raster order, texel f at
// frame coordinates (x0 + f % kFoot, y0 + f / kFoot) -- outside the frame along its borders.  at(px, py): the texel of a pixel of the tile; its neighbour
// (dx, dy), |dx|, |dy| <= R, lies dy * kFoot + dx further on.  tests/hostkernel/tiles_host.cpp checks that arithmetic on the host.
template <int32_t R>
struct TileWindow {
    static constexpr int32_t kFoot = 16 + 2 * R, kTexels = kFoot * kFoot;
    int32_t x0, y0;
    VR_HD static TileWindow of(int32_t tile, int32_t W) { const int32_t nx = tiles_x(W); return TileWindow{ (tile % nx) * 16 - R, (tile / nx) * 16 - R }; }
    VR_HD int32_t at(int32_t px, int32_t py) const { return (py - y0) * kFoot + (px - x0); }
};

// The window of a hi tile in a frame F times smaller per axis (vr_upsample.h): the lo texels that the 4 x 4 taps of the tile's 16 x 16 hi pixels can touch.  Hi
// pixel x has its taps at x0 - 1 .. x0 + 2 with x0 = floor((2x + 1 - F) / 2F) (upsample_split), so the window starts one below the x0 of the tile's first
// pixel and ends two above that of its last: kFoot = ceil(30 / 2F) + 4 texels per axis at most, whatever the tile (12, 9, 8 for F = 2, 3, 4).  Texel order and
// at() as in TileWindow, in lo coordinates; of() takes the HI frame's width.  tests/hostkernel/upsample_host.cpp checks the arithmetic on the host.
template <int32_t F>
struct ScaledTileWindow {
    static constexpr int32_t kFoot = (29 + 2 * F) / (2 * F) + 4, kTexels = kFoot * kFoot;
    int32_t x0, y0;
    VR_HD static int32_t first(int32_t hi) { return (2 * hi + 1 + F) / (2 * F) - 2; }      // x0 - 1 of hi coordinate `hi`, the floor taken of a positive numerator
    VR_HD static ScaledTileWindow of(int32_t tile, int32_t W) { const int32_t nx = tiles_x(W); return ScaledTileWindow{ first((tile % nx) * 16), first((tile / nx) * 16) }; }
    VR_HD int32_t at(int32_t lx, int32_t ly) const { return (ly - y0) * kFoot + (lx - x0); }
};

// The packed denoiser guides of the sharded renderer (pack_guides_kernel / unpack_guides_kernel): kGuidePlanes float4 planes per pixel -- 0 the moments
// texel, 1 and 2 the two float4 of the pixel's eight features -- plane-major inside a tile slot, thread t in raster_in_tile_pixel order.  The float4
// index below is WIRE FORMAT: the parts of a sharded renderer exchange these buffers, n_max * kGuidePlanes * 256 float4 per part.
// tests/hostkernel/guides_host.cpp builds it for the host.
constexpr uint32_t kGuidePlanes = 3u;
VR_HD size_t guide_slot(size_t tile_slot, uint32_t plane, uint32_t t) { return (tile_slot * kGuidePlanes + plane) * 256u + t; }

// Sample pool, one RGBA32F item per (pixel, sample) of a launch, written by the integrator kernels and read back by the accumulate kernel: the slot
// of lane `lane` of sub-tile `sub` of the launch's tile_slot-th tile, sample `sample` (0-based) of sample chunk `chunk`.  Work unit u = chunk * (n_tiles * 4) + (tile_slot * 4 + sub) owns the spu * 64 slots from u * spu * 64, sample-major.  I: the index
// type of the caller -- 32-bit in the path tracer (launch_pathtrace refuses a launch whose slots do not fit), size_t in the accumulate kernel
template <class I>
VR_HD I pool_slot(I chunk, int32_t n_tiles, I tile_slot, uint32_t sub, int32_t spu, I sample, uint32_t lane) {
    const I unit = chunk * ((I)n_tiles * 4u) + (tile_slot * 4u + sub);
    return unit * (I)(spu * 64) + sample * 64u + lane;
}

// Path-seed table of a renderer (renderer.h seed table; written by seed_fill_kernel, read by the path-tracing kernel's NEW batches): one uint32 per (sample
// number, pixel of the WHOLE frame in wave-tiled order).  s: the sample number as do_new hands it to the hash, minus the 1 a frame starts from; tile: the raster
// tile id of the whole frame (n_frame_tiles = tile_count(W, H)), so a launch over a tile subset reads the same entries as one over the frame.  The 64 lanes of a
// sub-tile are adjacent: a NEW batch, whose lanes take consecutive items, reads one or two contiguous 256-byte runs.  Pixels outside a ragged frame have entries
// (nobody reads them).  I: the caller's index type, as in pool_slot -- 32 bits in the kernels (the table is capped below 2^32 entries), size_t on the host
template <class I>
VR_HD I seed_table_index(I s, int32_t n_frame_tiles, I tile, uint32_t sub, uint32_t lane) {
    return ((s * (I)n_frame_tiles + tile) * 4u + sub) * 64u + lane;
}
// the sub-tile (0..3) of its 16x16 tile that holds pixel (px, py) -- the inverse of wave_tiled_pixel's sub
VR_HD uint32_t sub_of_pixel(int32_t px, int32_t py) { return (uint32_t)(((px >> 3) & 1) | (((py >> 3) & 1) << 1)); }

// unbiased variance = S * variance_scale(n) for n >= 2 samples, where S = Welford's M2 / n (the renderer's moments); 0 below (the callers give
// the variance itself as 0 there, not S * 0: S may be NaN)
VR_HD float variance_scale(int32_t n) { return n >= 2 ? (float)n / (float)(n - 1) : 0.0f; }

#if defined(__HIPCC__)
// a texel as the lane code takes it, float[4], and back: one dwordx4 either way
__device__ __forceinline__ void unpack4(const float4 t, float o[4]) { o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w; }
__device__ __forceinline__ float4 pack4(const float o[4]) { return make_float4(o[0], o[1], o[2], o[3]); }
// Fills win[0 .. kTexels) -- LDS of the workgroup of 256 threads that serves the window's tile -- with load(y * W + x) for a texel inside the W x H frame and
// off_value for any other, then waits for all of them.  EVERY thread of the workgroup calls it, before the `px >= W || py >= H` return of the threads whose
// pixel lies outside a ragged frame: they stage texels like the others, and the barrier counts them.
// Window: TileWindow<R>, or ScaledTileWindow<F> with W x H the lo frame.
template <class Window, class T, class Load>
__device__ __forceinline__ void stage_window(T* win, const Window window, int32_t W, int32_t H, const T off_value, Load load) {
    for (int32_t f = (int32_t)threadIdx.x; f < Window::kTexels; f += 256) {
        const int32_t x = window.x0 + f % Window::kFoot, y = window.y0 + f / Window::kFoot;
        T t = off_value;
        if (x >= 0 && x < W && y >= 0 && y < H) t = load(y * W + x);
        win[f] = t;
    }
    __syncthreads();
}
#endif

}  // namespace vr
