// vr_setup.hip -- scene and environment setup kernels (gfx950), run at commit() or when a setting changes, never per frame:
// the environment importance pyramid + warp table (env_setup.glsl, environment.cpp), the dense->brick encoder (voldata to_brick_grid at
// commit()) with its range mips, the paired and the decoded atlas, the majorant tables, and the clear-distance table of the expected-value pass.
#include <hip/hip_runtime.h>

#include "vr_clear.h"
#include "vr_device.h"
#include "vr_trace.h"

namespace vr {

// environment importance pyramid (env_setup.glsl:18-34; DIMENSION 512, SAMPLES 64: environment.cpp:6-7)
__global__ void __launch_bounds__(256)
impmap_base_kernel(const float* __restrict__ envmap, int32_t env_w, int32_t env_h, int32_t dim, float* __restrict__ out) {
    const int32_t px = blockIdx.x * 16 + (threadIdx.x & 15), py = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (px >= dim || py >= dim) return;
    SceneParams P;                    // only the envmap view is used by env_texture
    P.envmap = envmap; P.env_rgbe = nullptr; P.env_w = env_w; P.env_h = env_h;      // (the pyramid is built from the float map: every other field stays unset)
    const int32_t ns = 8;
    const float inv_samples = 1.0f / (float)(ns * ns);
    const float oss = (float)(dim * ns);
    float importance = 0.0f;
    for (int32_t y = 0; y < ns; ++y)
        for (int32_t x = 0; x < ns; ++x) {
            const float u = ((float)(px * ns) + ((float)x + 0.5f)) / oss;
            const float v = ((float)(py * ns) + ((float)y + 0.5f)) / oss;
            importance += luma(env_texture(P, u, v));
        }
    out[(size_t)py * dim + px] = importance * inv_samples;
}
// glGenerateMipmap on R32F: 2x2 box, ((t00 + t10) + (t01 + t11)) * 0.25
__global__ void __launch_bounds__(256)
impmap_mip_kernel(const float* __restrict__ src, int32_t d, float* __restrict__ dst) {
    const int32_t hd = d >> 1;
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hd * hd) return;
    const int32_t x = i % hd, y = i / hd;
    const float a = src[(size_t)(2 * y) * d + 2 * x], b = src[(size_t)(2 * y) * d + 2 * x + 1];
    const float c = src[(size_t)(2 * y + 1) * d + 2 * x], e = src[(size_t)(2 * y + 1) * d + 2 * x + 1];
    dst[i] = ((a + b) + (c + e)) * 0.25f;
}
// warp table of sample_environment (see vr_trace.h; layout: vr_scene.h env_cdf_index): one thread per 2x2 block of pyramid
// level `mip` = one record of table level k = top - mip
__global__ void __launch_bounds__(256)
env_cdf_kernel(const float* __restrict__ level, int32_t d, int32_t top, int32_t k, float* __restrict__ table, uint32_t* __restrict__ unsafe) {
    const int32_t hd = d >> 1;
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hd * hd) return;
    const int32_t x = i % hd, y = i / hd;
    const float w0 = level[(size_t)(2 * y) * d + 2 * x], w1 = level[(size_t)(2 * y) * d + 2 * x + 1];
    const float w2 = level[(size_t)(2 * y + 1) * d + 2 * x], w3 = level[(size_t)(2 * y + 1) * d + 2 * x + 1];
    const float q0 = w0 + w2, q1 = w1 + w3;
    float* o = table + env_cdf_index(top, k, (uint32_t)x, (uint32_t)y);
    o[0] = q0 / max_(1e-8f, q0 + q1); o[1] = w0 / q0; o[2] = w1 / q1;
    // may sample_environment's quotients use div_core (vr_math.h)?  Every threshold NaN (0 / 0 of an empty block: NaN either way), 0, or in [2^-76, 1]
    bool ok = true;
    for (int j = 0; j < 3; ++j) { const float v = o[j]; ok = ok && (v != v || v == 0.0f || (v >= 1.3234890e-23f && v <= 1.0f)); }
    if (!ok) atomicOr(unsafe, 1u);
    if (k == top) { o[3] = w0; o[4] = w1; o[5] = w2; o[6] = w3; }      // finest level: the texels themselves (pdf of the sampled direction)
}
void launch_build_env_cdf(const float* pyramid, int32_t dim, float* table, uint32_t* unsafe_flag, hipStream_t stream) {
    // levels base-1 .. 0; level m lives at pyramid offset imp_level_offset(dim, m) and has (dim >> m)^2 texels
    int32_t base = 0;
    while ((1 << base) < dim) ++base;
    (void)hipMemsetAsync(table, 0, env_cdf_table_floats(base - 1) * sizeof(float), stream);      // padding words and unused child records
    (void)hipMemsetAsync(unsafe_flag, 0, sizeof(uint32_t), stream);
    for (int32_t mip = base - 1; mip >= 0; --mip) {
        const int32_t d = dim >> mip, n = (d >> 1) * (d >> 1);
        hipLaunchKernelGGL(env_cdf_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, pyramid + imp_level_offset(dim, mip), d, base - 1, base - 1 - mip, table, unsafe_flag);
    }
}

void launch_build_impmap(const float* envmap_rgba, int32_t env_w, int32_t env_h, int32_t dim, float* pyramid, hipStream_t stream) {
    const dim3 grid((dim + 15) / 16, (dim + 15) / 16), block(256);
    hipLaunchKernelGGL(impmap_base_kernel, grid, block, 0, stream, envmap_rgba, env_w, env_h, dim, pyramid);
    float* src = pyramid;
    for (int32_t d = dim; d > 1; d >>= 1) {
        float* dst = src + (size_t)d * d;
        const int32_t n = (d >> 1) * (d >> 1);
        hipLaunchKernelGGL(impmap_mip_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, d, dst);
        src = dst;
    }
}

// ---------------------------------------------------------------------------------------------------
// Dense -> brick encoder on the device (voldata's Volume::to_brick_grid, commit() step of the reference:
// src/renderer.cpp:63).  Same rules, same arithmetic and same slot order as the host encoder in grids.cpp, so both
// produce identical device arrays (tests compare checksums):
//   1. encode_range_kernel : per brick, (min, max) over the brick dilated by 2 voxels, rounded outwards to fp16;
//                            flag = the brick's voxels matter (max != min)
//   2. encode_brick_kernel : per brick, BrickRec + 512 quantised voxels straight into its block of the brick-linear atlas (5 lines of range + 120 voxels: vr_scene.h)
//   3. range_mip_kernel    : (min of mins, max of maxes) over 2x2x2 children, three levels
__global__ void __launch_bounds__(256)
encode_range_kernel(const float* __restrict__ dense, int32_t nx, int32_t ny, int32_t nz, int32_t nbx, int32_t nby, int32_t nbz,
                    uint32_t* __restrict__ range, uint32_t* __restrict__ flag) {
    // one wavefront per brick: 12^3 = 1728 taps, 27 per lane
    const int32_t brick = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (brick >= nbx * nby * nbz) return;
    const int32_t bx = brick % nbx, by = (brick / nbx) % nby, bz = brick / (nbx * nby);
    const int32_t x0 = bx * 8 - 2, y0 = by * 8 - 2, z0 = bz * 8 - 2;
    float lo = inf_(), hi = -inf_();
    if (x0 >= nx || y0 >= ny || z0 >= nz) { lo = hi = 0.0f; }
    else
        for (int32_t i = lane; i < 1728; i += 64) {
            const int32_t x = x0 + i % 12, y = y0 + (i / 12) % 12, z = z0 + i / 144;
            float v = 0.0f;
            if (x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz) v = dense[((size_t)z * ny + y) * nx + x];
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
    for (int32_t o = 32; o > 0; o >>= 1) {
        const float l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) {
        // a zero bound is +0.0, as in the host encoder (grids.cpp): which of -0.0 and +0.0 the reduction ends on depends on its order
        if (lo == 0.0f) lo = 0.0f;
        if (hi == 0.0f) hi = 0.0f;
        const uint32_t hlo = float_to_half_down(lo), hhi = float_to_half_up(hi);
        range[brick] = hlo | (hhi << 16);
        flag[brick] = half2float(hhi) != half2float(hlo) ? 1u : 0u;
    }
}
__global__ void __launch_bounds__(64)
encode_brick_kernel(const float* __restrict__ dense, int32_t nx, int32_t ny, int32_t nz, int32_t nbx, int32_t nby,
                    const uint32_t* __restrict__ range, const uint32_t* __restrict__ flag,
                    BrickRec* __restrict__ recs, float* __restrict__ rng, uint8_t* __restrict__ atlas) {
    const int32_t brick = blockIdx.x, lane = threadIdx.x;
    const int32_t bx = brick % nbx, by = (brick / nbx) % nby, bz = brick / (nbx * nby);
    const uint32_t rg = range[brick];
    const float lo = half2float(rg & 0xFFFFu), hi = half2float(rg >> 16);
    const bool alloc = flag[brick] != 0u;                    // a brick whose range is one value keeps its zeroed block
    const size_t idx = ((size_t)bz * nby + by) * nbx + bx;            // brick-linear atlas: block index = record index = linear brick index
    if (lane == 0) { BrickRec r; r.slot = (uint32_t)idx; r.rmin = lo; r.rdiff = hi - lo; r.range = rg; recs[idx] = r; rng[2 * idx] = r.rmin; rng[2 * idx + 1] = r.rdiff; }
    uint8_t* dst = atlas + idx * (size_t)kBrickBlockBytes;
    if (VR_BRICK_HEADERS && lane < 5) { float* h = reinterpret_cast<float*>(dst + lane * 128); h[0] = lo; h[1] = hi - lo; }      // every line of every brick carries the range
    if (!alloc) return;
    const float inv = 255.0f / (hi - lo);
    for (int32_t i = lane; i < 512; i += 64) {
        const int32_t x = bx * 8 + (i & 7), y = by * 8 + ((i >> 3) & 7), z = bz * 8 + (i >> 6);
        float v = 0.0f;
        if (x < nx && y < ny && z < nz) v = dense[((size_t)z * ny + y) * nx + x];
        float qv = floor_((v - lo) * inv + 0.5f);
        qv = qv > 0.0f ? (qv > 255.0f ? 255.0f : qv) : 0.0f;      // clamp to [0, 255]; NaN becomes a defined 0, as in the host encoder (grids.cpp)
        dst[brick_voxel_byte((uint32_t)i)] = (uint8_t)qv;
    }
}
__global__ void __launch_bounds__(256)
range_mip_kernel(const uint32_t* __restrict__ src, int32_t sx, int32_t sy, int32_t sz, uint32_t* __restrict__ dst, int32_t dx, int32_t dy, int32_t dz) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dx * dy * dz) return;
    const int32_t x = i % dx, y = (i / dx) % dy, z = i / (dx * dy);
    float lo = inf_(), hi = -inf_(); uint32_t hlo = 0u, hhi = 0u;
    for (int32_t c = 0; c < 8; ++c) {
        const int32_t cx = 2 * x + (c & 1), cy = 2 * y + ((c >> 1) & 1), cz = 2 * z + (c >> 2);
        if (cx >= sx || cy >= sy || cz >= sz) continue;
        const uint32_t rg = src[((size_t)cz * sy + cy) * sx + cx];
        const float l = half2float(rg & 0xFFFFu), h = half2float(rg >> 16);
        if (l < lo) { lo = l; hlo = rg & 0xFFFFu; }
        if (h > hi) { hi = h; hhi = rg >> 16; }
    }
    dst[i] = hlo | (hhi << 16);
}

void launch_encode_ranges(const float* dense, const int32_t dim[3], const int32_t nb[3], uint32_t* range, uint32_t* flag, hipStream_t stream) {
    const int32_t n = nb[0] * nb[1] * nb[2];
    hipLaunchKernelGGL(encode_range_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, dense, dim[0], dim[1], dim[2], nb[0], nb[1], nb[2], range, flag);
}
void launch_encode_bricks(const float* dense, const int32_t dim[3], const int32_t nb[3], const uint32_t* range, const uint32_t* flag,
                          BrickRec* recs, float* rng, uint8_t* atlas, hipStream_t stream) {
    const int32_t n = nb[0] * nb[1] * nb[2];
    hipLaunchKernelGGL(encode_brick_kernel, dim3(n), dim3(64), 0, stream, dense, dim[0], dim[1], dim[2], nb[0], nb[1], range, flag, recs, rng, atlas);
}
void launch_range_mip(const uint32_t* src, const int32_t sdim[3], uint32_t* dst, const int32_t ddim[3], hipStream_t stream) {
    const int32_t n = ddim[0] * ddim[1] * ddim[2];
    hipLaunchKernelGGL(range_mip_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, src, sdim[0], sdim[1], sdim[2], dst, ddim[0], ddim[1], ddim[2]);
}

// paired atlas (vr_scene.h): the voxels of a density brick and of the emission brick at the same index, interleaved, with both decode ranges at the head of every line
__global__ void __launch_bounds__(64)
pair_atlas_kernel(const uint8_t* __restrict__ atlas_d, const uint8_t* __restrict__ atlas_e, uint8_t* __restrict__ out) {
    const size_t rec = blockIdx.x;
    const uint8_t* bd = atlas_d + rec * (size_t)kBrickBlockBytes;
    const uint8_t* be = atlas_e + rec * (size_t)kBrickBlockBytes;
    uint8_t* dst = out + rec * (size_t)kPairBlockBytes;
    const int32_t lane = threadIdx.x;
    if (lane < 10) {          // every line's header: (rmin, rdiff) of both bricks = the first 8 bytes of any line of their own blocks
        const float* hd = reinterpret_cast<const float*>(bd);
        const float* he = reinterpret_cast<const float*>(be);
        float* h = reinterpret_cast<float*>(dst + lane * 128);
        h[0] = hd[0]; h[1] = hd[1]; h[2] = he[0]; h[3] = he[1];
    }
    for (int32_t i = lane; i < 512; i += 64) {
        dst[pair_voxel_byte((uint32_t)i, 0u)] = bd[brick_voxel_byte((uint32_t)i)];
        dst[pair_voxel_byte((uint32_t)i, 1u)] = be[brick_voxel_byte((uint32_t)i)];
    }
}
void launch_pair_atlas(const uint8_t* atlas_d, const uint8_t* atlas_e, uint8_t* out, size_t n_records, hipStream_t stream) {
    if (n_records == 0) return;
    hipLaunchKernelGGL(pair_atlas_kernel, dim3((unsigned)n_records), dim3(64), 0, stream, atlas_d, atlas_e, out);
}

// decoded float atlas for transfer-function renders: out[i*512 + v] = rmin_i + unorm8(atlas[i*512 + v]) * rdiff_i (common.glsl:268-275)
__global__ void __launch_bounds__(256)
decode_atlas_kernel(const float* __restrict__ rng, const uint8_t* __restrict__ atlas, float* __restrict__ out, size_t n_voxels) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_voxels) return;
    const size_t cell = i >> 9;
    out[i] = rng[2 * cell] + unorm8(atlas[cell * (size_t)kBrickBlockBytes + brick_voxel_byte((uint32_t)(i & 511u))]) * rng[2 * cell + 1];
}
void launch_decode_atlas(const float* rng, const uint8_t* atlas, float* out, size_t n_records, hipStream_t stream) {
    const size_t n = n_records * 512u;
    if (n == 0) return;
    hipLaunchKernelGGL(decode_atlas_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, stream, rng, atlas, out, n);
}

// ---------------------------------------------------------------------------------------------------
// effective majorant of every cell of every level, written in the padded power-of-two layout that majorant_at indexes
// (vr_scene.h); cells beyond a level's real extent -- and levels the grid does not have -- hold 0
struct MajorantLayout { int32_t nb[3], mip_off[4], n_mips, mshift[3], blocked; };
__global__ void __launch_bounds__(256)
majorant_kernel(const SceneParams P, const uint32_t* __restrict__ range_words, const MajorantLayout L, uint32_t n_padded, float* __restrict__ out, uint16_t* __restrict__ out16) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n_padded) return;                                 // cell n_padded: "outside the grid" (vr_scene.h majorant_table_cells)
    const uint32_t k = (uint32_t)(L.mshift[0] + L.mshift[1] + L.mshift[2]);
    uint32_t mip = 0u;
    while (mip < 3u && i >= majorant_level_offset(k, mip + 1u)) ++mip;
    const uint32_t j = i - majorant_level_offset(k, mip);
    const uint32_t sx = (uint32_t)L.mshift[0] - mip, sy = (uint32_t)L.mshift[1] - mip;
    uint32_t cx, cy, cz;                                   // invert majorant_cell_index: which cell lives at position j of this level
    if (L.blocked && mip <= 1u) {
        const uint32_t blk = j >> 6, in = j & 63u;
        cx = ((blk & ((1u << (sx - 2u)) - 1u)) << 2) | (in & 3u);
        cy = (((blk >> (sx - 2u)) & ((1u << (sy - 2u)) - 1u)) << 2) | ((in >> 2) & 3u);
        cz = ((blk >> (sx + sy - 4u)) << 2) | (in >> 4);
    } else { cx = j & ((1u << sx) - 1u); cy = (j >> sx) & ((1u << sy) - 1u); cz = j >> (sx + sy); }
    const uint32_t rnd = (1u << mip) - 1u;
    const uint32_t dx = ((uint32_t)L.nb[0] + rnd) >> mip, dy = ((uint32_t)L.nb[1] + rnd) >> mip, dz = ((uint32_t)L.nb[2] + rnd) >> mip;
    // a cell beyond the level's real extent, a level the grid does not have and the table's last cell read what the reference's out-of-range texelFetch
    // returns, 0, and go through the same arithmetic: density_scale * 0, TF-remapped when a LUT is bound (common.glsl:278-281, 425)
    uint32_t h = 0u;
    if (i < n_padded && (int32_t)mip <= L.n_mips && cx < dx && cy < dy && cz < dz)
        h = range_words[(uint32_t)L.mip_off[mip] + (cz * dy + cy) * dx + cx] >> 16;
    float m = P.u.vol_density_scale * half2float(h);
    if (P.u.use_tf) {
        float rgba[4];
        tf_lookup(P, m * P.u.vol_inv_majorant, rgba);
        m = P.u.vol_majorant * rgba[3];
    }
    out[i] = m;
    out16[i] = (uint16_t)h;
}
void launch_majorants(const SceneParams& P, const uint32_t* range_words_all_mips, const int32_t nb[3], const int32_t mip_off[4], int32_t n_mips,
                      const int32_t mshift[3], float* out_padded, uint16_t* out16_padded, hipStream_t stream) {
    MajorantLayout L;
    L.blocked = P.density.maj_blocked;
    for (int i = 0; i < 3; ++i) { L.nb[i] = nb[i]; L.mshift[i] = mshift[i]; }
    for (int i = 0; i < 4; ++i) L.mip_off[i] = mip_off[i];
    L.n_mips = n_mips;
    const uint32_t n = (uint32_t)majorant_padded_cells((uint32_t)(mshift[0] + mshift[1] + mshift[2]));
    hipLaunchKernelGGL(majorant_kernel, dim3((n + 256u) / 256u), dim3(256), 0, stream, P, range_words_all_mips, L, n, out_padded, out16_padded);      // n + 1 cells
}

// ---------------------------------------------------------------------------------------------------
// Clear-distance table of a density grid (vr_clear.h), built at the first expected-value pass that reads the grid.
//   1. clear_mark_kernel : one wavefront per cell, the 10^3 (reach 1) or 12^3 (reach 2) voxels of its grown box spread over the lanes; 255 when all of them are +0, else 0
//   2. clear_axis_kernel : one thread per cell, once per axis (x, y, z), each from one buffer into the other
__global__ void __launch_bounds__(256)
clear_mark_kernel(const GridView g, int32_t n0, int32_t n1, int32_t n2, int32_t reach, uint8_t* __restrict__ out) {
    const uint32_t cell = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (cell >= (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2) return;                    // the whole wavefront
    const int32_t cx = (int32_t)(cell % (uint32_t)n0), cy = (int32_t)((cell / (uint32_t)n0) % (uint32_t)n1), cz = (int32_t)(cell / ((uint32_t)n0 * (uint32_t)n1));
    const uint32_t bits = clear_box_bits(g, cx, cy, cz, (int32_t)lane, 64, reach);
    const bool any = __ballot(bits != 0u) != 0ull;
    if (lane == 0u) out[cell] = any ? (uint8_t)0 : (uint8_t)kClearMax;
}
__global__ void __launch_bounds__(256)
clear_axis_kernel(const uint8_t* __restrict__ in, int32_t n0, int32_t n1, int32_t n2, int32_t axis, uint8_t* __restrict__ out) {
    const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= (uint32_t)n0 * (uint32_t)n1 * (uint32_t)n2) return;
    const int32_t n[3] = { n0, n1, n2 };
    const int32_t cx = (int32_t)(cell % (uint32_t)n0), cy = (int32_t)((cell / (uint32_t)n0) % (uint32_t)n1), cz = (int32_t)(cell / ((uint32_t)n0 * (uint32_t)n1));
    out[cell] = (uint8_t)clear_axis_pass(in, n, axis, cx, cy, cz);
}
void launch_clear_table(const GridView& g, uint8_t* table, uint8_t* scratch, hipStream_t stream, int32_t reach) {
    int32_t n[3];
    clear_cells(g, n);
    const uint32_t cells = (uint32_t)n[0] * (uint32_t)n[1] * (uint32_t)n[2];
    if (cells == 0u) return;
    hipLaunchKernelGGL(clear_mark_kernel, dim3((cells + 3u) / 4u), dim3(256), 0, stream, g, n[0], n[1], n[2], reach == 2 ? 2 : 1, scratch);
    const dim3 grid((cells + 255u) / 256u);
    hipLaunchKernelGGL(clear_axis_kernel, grid, dim3(256), 0, stream, scratch, n[0], n[1], n[2], 0, table);
    hipLaunchKernelGGL(clear_axis_kernel, grid, dim3(256), 0, stream, table, n[0], n[1], n[2], 1, scratch);
    hipLaunchKernelGGL(clear_axis_kernel, grid, dim3(256), 0, stream, scratch, n[0], n[1], n[2], 2, table);
}

// Path-seed table: one thread per entry of the sample numbers [s_begin, s_begin + n) (vr_device.h launch_seed_fill).  Consecutive threads write consecutive entries.
__global__ void __launch_bounds__(256)
seed_fill_kernel(uint32_t* __restrict__ table, uint32_t seed, int32_t W, int32_t n_tiles, uint32_t s_begin, size_t n_entries) {
    const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (g >= n_entries) return;
    const size_t per_sample = (size_t)n_tiles * 256u;
    const uint32_t s = s_begin + (uint32_t)(g / per_sample), r = (uint32_t)(g % per_sample);
    const TilePixel q = wave_tiled_pixel((int32_t)(r >> 8), r & 255u, W);
    table[seed_table_index<size_t>(s, n_tiles, (size_t)q.tile, (uint32_t)q.sub, (uint32_t)q.lane)] = path_seed(seed, W, q.px, q.py, (int32_t)s + 1);
}
void launch_seed_fill(uint32_t* table, uint32_t seed, int32_t W, int32_t H, int32_t s_begin, int32_t s_end, hipStream_t stream) {
    if (s_end <= s_begin || s_begin < 0) return;
    const int32_t n_tiles = tile_count(W, H);
    const size_t n_entries = (size_t)(s_end - s_begin) * (size_t)n_tiles * 256u;
    hipLaunchKernelGGL(seed_fill_kernel, dim3((unsigned)((n_entries + 255u) / 256u)), dim3(256), 0, stream, table, seed, W, n_tiles, (uint32_t)s_begin, n_entries);
}

}  // namespace vr
