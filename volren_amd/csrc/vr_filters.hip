// vr_filters.hip -- the image-space kernels (gfx950): everything that reads or writes whole frames or tiles of them after the path tracer.
// The a-trous denoiser (vr_denoise.h: prepare, iterations) with its temporal accumulation (vr_temporal.h, vr_moments.h), the error estimate of adaptive
// sampling (vr_adaptive.h), the control variate on the expected coverage (vr_resolve.h), the layered filter's split and merge (vr_layers.h), its one-pass regression (vr_regress.h), the layer's upsampling under a full-resolution guide (vr_upsample.h), tonemap.glsl, and tile pack / unpack for the multi-GPU gather.  One thread per pixel; the per-pixel kernels use
// the wave-tiled layout of vr_tiles.h (16x16 tiles of four 8x8 wavefronts, like the accumulate kernel) for the 2-D locality of their footprints.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "vr_adaptive.h"
#include "vr_demod.h"
#include "vr_denoise.h"
#include "vr_device.h"
#include "vr_layers.h"
#include "vr_moments.h"
#include "vr_regress.h"
#include "vr_resolve.h"
#include "vr_temporal.h"
#include "vr_upsample.h"

namespace vr {

// Denoiser (vr_denoise.h).  No LDS: from step 4 on the 5x5 footprint leaves the tile, and the working set fits the Infinity Cache.  Per tap: the
// colour (one dwordx4), the variance (one dword) and the guide (two dwordx4).
struct GuideDev {          // the guide by pixel index, also for pass 2 of vr_moments.h
    const float4* __restrict__ g;
    __device__ __forceinline__ void guide(int32_t i, float o[8]) const { const float4 a = g[2 * i], b = g[2 * i + 1]; unpack4(a, o); unpack4(b, o + 4); }
};
struct DenoiseSrcDev : GuideDev {
    const float4* __restrict__ c;
    const float* __restrict__ v;
    __device__ __forceinline__ void color(int32_t i, float o[4]) const { unpack4(c[i], o); }
    __device__ __forceinline__ float var(int32_t i) const { return v[i]; }
};
// prepare: moments S (W*H*4, Welford's M2 / n) -> the unbiased variance var = S * vscale exactly as vr_variance forms it (0 for n = 1), then
// the variance of the mean's luminance v (W*H) and the guide (W*H*8) from the features.  counts (a frame of adaptive sampling: one count per
// raster tile) replaces the scalar n and vscale with the tile's own, formed as the host forms vscale; nullptr = the scalars.  DEMOD ("denoise_demodulate" = 1):
// v is vr_demod.h's, the variance of the layer divided by the albedo the pixel's features already hold in registers: three divisions more, no load more
template <bool DEMOD>
__global__ void __launch_bounds__(256)
denoise_prepare_kernel(const float4* __restrict__ moments, const float4* __restrict__ features, int32_t W, int32_t H, int32_t n_all, float vscale_all,
                       const int32_t* __restrict__ counts, float* __restrict__ v, float4* __restrict__ guide) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const int32_t n = counts ? counts[q.tile] : n_all;
    const float vscale = counts ? variance_scale(n) : vscale_all;
    const int32_t i = q.py * W + q.px;
    const float4 m = moments[i];
    const float var[4] = { n >= 2 ? m.x * vscale : 0.0f, n >= 2 ? m.y * vscale : 0.0f, n >= 2 ? m.z * vscale : 0.0f, n >= 2 ? m.w * vscale : 0.0f };
    const float4 fa = features[2 * i], fb = features[2 * i + 1];
    float f[8], g[8];
    unpack4(fa, f); unpack4(fb, f + 4);
    denoise_guide(f, g);
    if constexpr (DEMOD) v[i] = demod_mean_variance(var, f, n);
    else v[i] = denoise_mean_variance(var, n);
    guide[2 * i] = pack4(g);
    guide[2 * i + 1] = pack4(g + 4);
}
// one a-trous iteration; vout == nullptr: the variance is not written (the last iteration)
__global__ void __launch_bounds__(256)
denoise_atrous_kernel(const float4* __restrict__ cin, const float* __restrict__ vin, const float4* __restrict__ guide, int32_t W, int32_t H,
                      int32_t step, const DenoiseSigma sg, float4* __restrict__ cout, float* __restrict__ vout) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const DenoiseSrcDev src{ { guide }, cin, vin };
    float o[4], ov;
    denoise_atrous_pixel(src, W, H, q.px, q.py, step, sg, o, ov);
    const int32_t i = q.py * W + q.px;
    cout[i] = pack4(o);
    if (vout) vout[i] = ov;
}
void launch_denoise_prepare(const float* moments, const float* features, int32_t W, int32_t H, int32_t n, float vscale, const int32_t* counts, float* v, float* guide,
                            hipStream_t stream, bool demod) {
    if (W <= 0 || H <= 0) return;
    hipLaunchKernelGGL((demod ? denoise_prepare_kernel<true> : denoise_prepare_kernel<false>), dim3((unsigned)tile_count(W, H)), dim3(256), 0, stream,
                       reinterpret_cast<const float4*>(moments), reinterpret_cast<const float4*>(features), W, H, n, vscale, counts, v, reinterpret_cast<float4*>(guide));
}
void launch_denoise_atrous(const float* cin, const float* vin, const float* guide, int32_t W, int32_t H, int32_t step, const DenoiseSigma& sg,
                           float* cout, float* vout, hipStream_t stream) {
    if (W <= 0 || H <= 0) return;
    hipLaunchKernelGGL(denoise_atrous_kernel, dim3((unsigned)tile_count(W, H)), dim3(256), 0, stream, reinterpret_cast<const float4*>(cin), vin,
                       reinterpret_cast<const float4*>(guide), W, H, step, sg, reinterpret_cast<float4*>(cout), vout);
}

// Temporal accumulation (vr_temporal.h temporal_pixel), between prepare and the iterations.
// Reads the pixel's colour, v and the guide's coverage and depth (52 B), gathers up to four taps of the previous history -- a tap is two dwordx4:
// the colour and (V, N, K, D), fetched only after the tap was found inside the frame -- and writes the pixel's new history (32 B) into the other
// half of the ping-pong pair, plus V over the pixel's own v, where the iterations read it.  No LDS, no atomics; the only loops are the 2 x 2 taps.
struct TemporalHistDev {
    const float4* __restrict__ c;
    const float4* __restrict__ s;
    __device__ __forceinline__ void color(int32_t i, float o[4]) const { unpack4(c[i], o); }
    __device__ __forceinline__ void record(int32_t i, float o[4]) const { unpack4(s[i], o); }
};
// MOMENTS (vr_moments.h pass 1, "denoise_moments" = 1): every tap that counts also gives its moment record (a third dwordx4), the pixel's new moment
// record goes to om (16 B more), and v is left alone: denoise_moments_variance_kernel writes it.  false: hm, om are not touched.
struct MomentsHistDev {
    const float4* __restrict__ m;
    __device__ __forceinline__ void moments(int32_t i, float o[4]) const { unpack4(m[i], o); }
};
template <bool MOMENTS>
__global__ void __launch_bounds__(256)
denoise_temporal_kernel(const float4* __restrict__ color, float* __restrict__ v, const float4* __restrict__ guide, const float4* __restrict__ hc,
                        const float4* __restrict__ hs, const float4* __restrict__ hm, int32_t have, int32_t same_cam, const TemporalCamera cur,
                        const TemporalCamera prev, int32_t W, int32_t H, float alpha, float4* __restrict__ oc, float4* __restrict__ os, float4* __restrict__ om) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float c[4];
    unpack4(color[i], c);
    const TemporalHistDev hist{ hc, hs };
    float C[4], S[4];
    if constexpr (MOMENTS) {
        float M[4];
        moments_pixel(hist, MomentsHistDev{ hm }, have != 0, same_cam != 0, cur, prev, W, H, q.px, q.py, c, guide[2 * i].w, guide[2 * i + 1].w, alpha, C, S, M);
        om[i] = pack4(M);
    } else {
        temporal_pixel(hist, have != 0, same_cam != 0, cur, prev, W, H, q.px, q.py, c, v[i], guide[2 * i].w, guide[2 * i + 1].w, alpha, C, S);
    }
    oc[i] = pack4(C);
    os[i] = pack4(S);
    if constexpr (!MOMENTS) v[i] = S[0];
}

// Pass 2 of vr_moments.h: the variance of the filter's input from the moments pass 1 blended.  Stages (m1, m2) of the tile's 22 x 22 footprint (16 x 16
// plus a halo of 3; one dwordx2 load per pixel, m2 = -1 "off the frame") in 3872 B of LDS, one barrier -- threads outside the frame stage and wait with
// the others -- then a pixel with N >= 4 reads its own pair back, and only a pixel with a shorter history runs the 49 taps.  The guide taps come straight
// from global memory, as the a-trous kernel reads them, not from LDS: after the first frames only disoccluded pixels pool, and staging 22 x 22 x 32 B of
// guide per tile would charge every tile of every frame 15 KiB of loads for taps that almost none of its pixels make; on the first frame, where all do,
// the 49 x 32 B of a pixel are its neighbours' too and hit the L2.  Writes S into the pixel's moment record, V = S * E into its history record and over
// its v: words of its own pixel that no other thread reads (the staging of the neighbouring tiles reads m1, m2 only, at no fixed time).  No atomics.
using MomentsWindow = TileWindow<kMomentsWindow>;
struct MomentsWindowDev {
    const float2* win;     // the staged footprint
    int32_t at;            // the pixel's own pair in it
    __device__ __forceinline__ void moments(int32_t dx, int32_t dy, float m[2]) const { const float2 p = win[at + dy * MomentsWindow::kFoot + dx]; m[0] = p.x; m[1] = p.y; }
};
__global__ void __launch_bounds__(256)
denoise_moments_variance_kernel(const float4* __restrict__ guide, int32_t W, int32_t H, const DenoiseSigma sg, float4* os, float4* om, float* __restrict__ v) {
    __shared__ float2 win[MomentsWindow::kTexels];
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    const MomentsWindow window = MomentsWindow::of((int32_t)blockIdx.x, W);
    stage_window(win, window, W, H, make_float2(0.0f, kMomentsOffFrame), [&](int32_t i) { return *reinterpret_cast<const float2*>(&om[i].x); });
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    const float N = os[i].y, E = om[i].z;
    const float S = moments_variance(MomentsWindowDev{ win, window.at(q.px, q.py) }, GuideDev{ guide }, W, q.px, q.py, N, sg);
    const float V = S * E;
    om[i].w = S;
    os[i].x = V;
    v[i] = V;
}

// The same with the rejection test (vr_temporal.h steps 2a, 3a; tau > 0 only), as two kernels, because a pixel's decision needs the z2 of its 5 x 5
// neighbours.  Between them lies a scratch pair of W*H float4 each: h, and (v_h, N_h, z2, has).
// fetch: today's gather (52 B in, up to four taps), then z2; writes the two dwordx4 of the scratch.
// resolve: stages the window words of the tile's 20 x 20 footprint (16 x 16 plus a halo of 2, one dwordx2 load per pixel, "no history" off the frame)
// in 1600 B of LDS, one barrier -- threads outside the frame stage and wait with the others -- then sums its 25 words from LDS, blends, and writes
// the new history and v where denoise_temporal_kernel writes them.  The statistic T (-1 without a history) goes over the pixel's v_h word, which only
// this thread reads: the z2 and has words are read by the neighbouring tiles' staging, at no fixed time, so they stay as they are.  No atomics.
using RejectWindow = TileWindow<kTemporalWindow>;
struct TemporalWindowDev {
    const float* win;      // the staged footprint
    int32_t at;            // the pixel's own word in it
    __device__ __forceinline__ float word(int32_t dx, int32_t dy) const { return win[at + dy * RejectWindow::kFoot + dx]; }
};
__global__ void __launch_bounds__(256)
denoise_temporal_fetch_kernel(const float4* __restrict__ color, const float* __restrict__ v, const float4* __restrict__ guide, const float4* __restrict__ hc,
                              const float4* __restrict__ hs, int32_t have, int32_t same_cam, const TemporalCamera cur, const TemporalCamera prev, int32_t W,
                              int32_t H, float4* __restrict__ sh, float4* __restrict__ sr) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float c[4];
    unpack4(color[i], c);
    const TemporalHistDev hist{ hc, hs };
    float h[4], vh, nh;
    const bool has = temporal_fetch(hist, have != 0, same_cam != 0, cur, prev, W, H, q.px, q.py, guide[2 * i].w, guide[2 * i + 1].w, h, vh, nh);
    const float z2 = has ? temporal_z2(h, vh, c, v[i]) : 0.0f;
    sh[i] = pack4(h);
    sr[i] = make_float4(vh, nh, z2, has ? 1.0f : 0.0f);
}
__global__ void __launch_bounds__(256)
denoise_temporal_resolve_kernel(const float4* __restrict__ color, float* __restrict__ v, const float4* __restrict__ guide, const float4* __restrict__ sh,
                                float4* sr, int32_t W, int32_t H, float alpha, float tau, float4* __restrict__ oc, float4* __restrict__ os) {
    __shared__ float win[RejectWindow::kTexels];
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    const RejectWindow window = RejectWindow::of((int32_t)blockIdx.x, W);
    stage_window(win, window, W, H, kTemporalNoHistory, [&](int32_t i) {
        const float2 zh = *reinterpret_cast<const float2*>(&sr[i].z);
        return temporal_window_word(zh.y != 0.0f, zh.x);
    });
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float c[4], h[4];
    unpack4(color[i], c);
    unpack4(sh[i], h);
    const float4 r = sr[i];
    const bool has = r.w != 0.0f;
    float T = kTemporalNoHistory;
    if (has) T = temporal_pool(TemporalWindowDev{ win, window.at(q.px, q.py) });
    float C[4], S[4];
    temporal_blend(has && !temporal_rejects(T, tau), h, r.x, r.y, c, v[i], guide[2 * i].w, guide[2 * i + 1].w, alpha, C, S);
    oc[i] = pack4(C);
    os[i] = pack4(S);
    v[i] = S[0];
    sr[i].x = T;
}
// The one launcher of the three forms (vr_device.h TemporalPass): what the struct carries picks the kernels.
void launch_denoise_temporal(const TemporalPass& t, hipStream_t stream) {
    const bool moments = t.out_moments != nullptr, reject = t.tau > 0.0f, have = t.hist_color != nullptr;
    if (moments && reject) throw std::invalid_argument("launch_denoise_temporal: moment records and rejection do not go together");
    if (reject && !t.scratch) throw std::invalid_argument("launch_denoise_temporal: rejection without a scratch buffer");
    if ((t.hist_record != nullptr) != have || (t.hist_moments != nullptr) != (have && moments))
        throw std::invalid_argument("launch_denoise_temporal: the history's pointers are not all set or all null");
    if (t.W <= 0 || t.H <= 0) return;
    const dim3 grid((unsigned)tile_count(t.W, t.H)), block(256);
    const float4 *color = reinterpret_cast<const float4*>(t.color), *guide = reinterpret_cast<const float4*>(t.guide);
    const float4 *hc = reinterpret_cast<const float4*>(t.hist_color), *hs = reinterpret_cast<const float4*>(t.hist_record), *hm = reinterpret_cast<const float4*>(t.hist_moments);
    float4 *oc = reinterpret_cast<float4*>(t.out_color), *os = reinterpret_cast<float4*>(t.out_record), *om = reinterpret_cast<float4*>(t.out_moments);
    const int32_t have_i = have ? 1 : 0, same_i = t.same_cam ? 1 : 0;
    if (moments) {
        hipLaunchKernelGGL(denoise_temporal_kernel<true>, grid, block, 0, stream, color, t.v, guide, hc, hs, hm, have_i, same_i, t.cur, t.prev, t.W, t.H, t.alpha, oc, os, om);
        hipLaunchKernelGGL(denoise_moments_variance_kernel, grid, block, 0, stream, guide, t.W, t.H, t.sigma, os, om, t.v);
    } else if (reject) {
        float4* sh = reinterpret_cast<float4*>(t.scratch);
        float4* sr = sh + (size_t)t.W * t.H;
        hipLaunchKernelGGL(denoise_temporal_fetch_kernel, grid, block, 0, stream, color, t.v, guide, hc, hs, have_i, same_i, t.cur, t.prev, t.W, t.H, sh, sr);
        hipLaunchKernelGGL(denoise_temporal_resolve_kernel, grid, block, 0, stream, color, t.v, guide, sh, sr, t.W, t.H, t.alpha, t.tau, oc, os);
    } else {
        hipLaunchKernelGGL(denoise_temporal_kernel<false>, grid, block, 0, stream, color, t.v, guide, hc, hs, hm, have_i, same_i, t.cur, t.prev, t.W, t.H, t.alpha, oc, os, om);
    }
}

// The control variate of vr_resolve.h, two kernels with the frames B and P (W*H float4 each) between them, because a pixel's coefficient pools the P of its
// 7 x 7 neighbours.
// prepare: the pixel's framebuffer texel in (one dwordx4), rays x rays environment lookups (none with the environment hidden), B and P out (two dwordx4).
// resolve: stages P of the tile's 22 x 22 footprint (16 x 16 plus a halo of 3, one dwordx4 load per texel; zeros off the frame, which the lane code never
// asks for) in 7744 B of LDS, one barrier -- threads outside the frame stage and wait with the others -- then reads the pixel's texels of the framebuffer and
// of B and the coverage word of its features, sums its 49 taps from LDS and writes one dwordx4.  The same kernel with the taps read from global memory, as the
// a-trous kernel reads its own, measured 53.5 us against 24.1 us at 1024 x 1024 (profiles/r13_resolve.txt) and was dropped.  No atomics, no scratch.
using ResolveWindow = TileWindow<kResolveWindow>;
struct ResolveWindowDev {
    const float4* win;     // the staged footprint
    int32_t at;            // the pixel's own texel in it
    __device__ __forceinline__ void tap(int32_t dx, int32_t dy, float o[4]) const { unpack4(win[at + dy * ResolveWindow::kFoot + dx], o); }
};
__global__ void __launch_bounds__(256)
resolve_prepare_kernel(const SceneParams P, const float4* __restrict__ fb, int32_t rays, float4* __restrict__ B, float4* __restrict__ Pq) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float x[4], b[4], p[4];
    unpack4(fb[i], x);
    resolve_prepare_pixel(x, resolve_background(P, q.px, q.py, rays), b, p);
    B[i] = pack4(b);
    Pq[i] = pack4(p);
}
__global__ void __launch_bounds__(256)
resolve_kernel(const float4* __restrict__ fb, const float4* __restrict__ features, const float4* __restrict__ B, const float4* __restrict__ Pq, int32_t W, int32_t H,
               float4* __restrict__ out) {
    __shared__ float4 win[ResolveWindow::kTexels];
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    const ResolveWindow window = ResolveWindow::of((int32_t)blockIdx.x, W);
    stage_window(win, window, W, H, make_float4(0.0f, 0.0f, 0.0f, 0.0f), [&](int32_t i) { return Pq[i]; });
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float x[4], b[4], y[4];
    unpack4(fb[i], x);
    unpack4(B[i], b);
    resolve_pixel(ResolveWindowDev{ win, window.at(q.px, q.py) }, W, H, q.px, q.py, x, b, features[2 * i].w, y);
    out[i] = pack4(y);
}
void launch_resolve(const SceneParams& P, const float* fb, const float* features, int32_t rays, float* B, float* Pq, float* out, hipStream_t stream) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    if (W <= 0 || H <= 0 || rays < 1) return;
    const dim3 grid((unsigned)tile_count(W, H)), block(256);
    hipLaunchKernelGGL(resolve_prepare_kernel, grid, block, 0, stream, P, reinterpret_cast<const float4*>(fb), rays, reinterpret_cast<float4*>(B),
                       reinterpret_cast<float4*>(Pq));
    hipLaunchKernelGGL(resolve_kernel, grid, block, 0, stream, reinterpret_cast<const float4*>(fb), reinterpret_cast<const float4*>(features),
                       reinterpret_cast<const float4*>(B), reinterpret_cast<const float4*>(Pq), W, H, reinterpret_cast<float4*>(out));
}

// The layered filter of vr_layers.h: split in front of the denoiser's kernels, merge behind them.  One thread per pixel, dwordx4 loads and stores, no LDS, no
// atomics.  split reads the pixel's texels of the resolved frame and of B and the first float4 of its features (the coverage word) and writes S: 64 B a pixel.
// merge reads the filter's output, B and the same float4 and writes the frame and the layer: 80 B a pixel.  DEMOD ("denoise_demodulate" = 1): vr_demod.h's split
// and merge, whose divisor comes from the albedo words of that float4 -- the same bytes, three divisions (split) or three multiplies (merge) more.
template <bool DEMOD>
__global__ void __launch_bounds__(256)
layers_split_kernel(const float4* __restrict__ y, const float4* __restrict__ B, const float4* __restrict__ features, int32_t W, int32_t H, float4* __restrict__ S) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float yy[4], b[4], s[4];
    unpack4(y[i], yy);
    unpack4(B[i], b);
    if constexpr (DEMOD) {
        float ak[4];
        unpack4(features[2 * i], ak);
        demod_split_pixel(yy, b, ak, s);
    } else {
        layers_split_pixel(yy, b, features[2 * i].w, s);
    }
    S[i] = pack4(s);
}
template <bool DEMOD>
__global__ void __launch_bounds__(256)
layers_merge_kernel(const float4* __restrict__ F, const float4* __restrict__ B, const float4* __restrict__ features, int32_t W, int32_t H, float4* __restrict__ out,
                    float4* __restrict__ L) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float f[4], b[4], l[4], o[4];
    unpack4(F[i], f);
    unpack4(B[i], b);
    if constexpr (DEMOD) {
        float ak[4];
        unpack4(features[2 * i], ak);
        demod_merge_pixel(f, b, ak, l, o);
    } else {
        layers_merge_pixel(f, b, features[2 * i].w, l, o);
    }
    out[i] = pack4(o);
    L[i] = pack4(l);
}
void launch_layers_split(const float* y, const float* B, const float* features, int32_t W, int32_t H, float* S, hipStream_t stream, bool demod) {
    if (W <= 0 || H <= 0) return;
    hipLaunchKernelGGL((demod ? layers_split_kernel<true> : layers_split_kernel<false>), dim3((unsigned)tile_count(W, H)), dim3(256), 0, stream, reinterpret_cast<const float4*>(y),
                       reinterpret_cast<const float4*>(B), reinterpret_cast<const float4*>(features), W, H, reinterpret_cast<float4*>(S));
}
void launch_layers_merge(const float* F, const float* B, const float* features, int32_t W, int32_t H, float* out, float* L, hipStream_t stream, bool demod) {
    if (W <= 0 || H <= 0) return;
    hipLaunchKernelGGL((demod ? layers_merge_kernel<true> : layers_merge_kernel<false>), dim3((unsigned)tile_count(W, H)), dim3(256), 0, stream, reinterpret_cast<const float4*>(F),
                       reinterpret_cast<const float4*>(B), reinterpret_cast<const float4*>(features), W, H, reinterpret_cast<float4*>(out),
                       reinterpret_cast<float4*>(L));
}

// The one-pass regression of vr_regress.h ("denoise_filter" = 1), in the place of the a-trous iterations: one workgroup per 16 x 16 tile.  Stages the tile's
// 26 x 26 footprint (16 x 16 plus a halo of 5) as records of three float4 -- S and the two float4 of the guide, 48 B a texel, 32448 B of static LDS: four
// workgroups, 16 waves, a CU -- once, one barrier; threads outside a ragged frame stage and wait with the others, and texels off the frame hold a record no tap
// reads (the lane code skips such taps by their coordinates).  Then a pixel runs its 121 taps from LDS, three ds_read_b128 a tap, with the 60 sums and the solve
// in registers, and writes one dwordx4.  The 48-byte records put the three reads of a 16-lane group two and three deep on some banks (MI355X: 64 banks, the
// row pitch 26 texels); a tap is some 300 VALU instructions -- the edge factors' pow_ and two exp_, the 60 multiply-add pairs -- against 12 LDS cycles without
// conflicts, so the layout is left as stage_window writes it.  VR_REGRESS_GLOBAL_TAPS = 1 builds the form whose taps read the three float4 from global memory
// instead (no LDS, no barrier), for comparison.  No atomics, no scratch.
#ifndef VR_REGRESS_GLOBAL_TAPS
#define VR_REGRESS_GLOBAL_TAPS 0
#endif
using RegressWindow = TileWindow<kRegressRadius>;
struct RegressTexel { float4 S, ga, gb; };
struct RegressWindowDev {
    const RegressTexel* win;     // the staged footprint
    int32_t at;                  // the pixel's own texel in it
    __device__ __forceinline__ void tap(int32_t dx, int32_t dy, float S[4], float g[8]) const {
        const RegressTexel& t = win[at + dy * RegressWindow::kFoot + dx];
        unpack4(t.S, S); unpack4(t.ga, g); unpack4(t.gb, g + 4);
    }
};
struct RegressGlobalDev {
    const float4* __restrict__ S;
    const float4* __restrict__ g;
    int32_t at, W;               // the pixel's own index, the frame's width
    __device__ __forceinline__ void tap(int32_t dx, int32_t dy, float Sq[4], float gq[8]) const {
        const int32_t i = at + dy * W + dx;
        unpack4(S[i], Sq); unpack4(g[2 * i], gq); unpack4(g[2 * i + 1], gq + 4);
    }
};
__global__ void __launch_bounds__(256)
denoise_regress_kernel(const float4* __restrict__ S, const float4* __restrict__ guide, int32_t W, int32_t H, const DenoiseSigma sg, float ridge, float4* __restrict__ F) {
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
#if !VR_REGRESS_GLOBAL_TAPS
    __shared__ RegressTexel win[RegressWindow::kTexels];
    const RegressWindow window = RegressWindow::of((int32_t)blockIdx.x, W);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    stage_window(win, window, W, H, RegressTexel{ zero, zero, zero }, [&](int32_t i) { return RegressTexel{ S[i], guide[2 * i], guide[2 * i + 1] }; });
#endif
    if (q.px >= W || q.py >= H) return;
    float f[4];
#if VR_REGRESS_GLOBAL_TAPS
    regress_pixel(RegressGlobalDev{ S, guide, q.py * W + q.px, W }, W, H, q.px, q.py, sg, ridge, f);
#else
    regress_pixel(RegressWindowDev{ win, window.at(q.px, q.py) }, W, H, q.px, q.py, sg, ridge, f);
#endif
    F[q.py * W + q.px] = pack4(f);
}
void launch_denoise_regress(const float* S, const float* guide, int32_t W, int32_t H, const DenoiseSigma& sg, float ridge, float* F, hipStream_t stream) {
    if (W <= 0 || H <= 0) return;
    hipLaunchKernelGGL(denoise_regress_kernel, dim3((unsigned)tile_count(W, H)), dim3(256), 0, stream, reinterpret_cast<const float4*>(S),
                       reinterpret_cast<const float4*>(guide), W, H, sg, ridge, reinterpret_cast<float4*>(F));
}

// The upsampling of vr_upsample.h: one workgroup per 16 x 16 tile of the HI frame, F = hi / lo per axis at compile time (the window's size and the divisions
// by 2F).  Stages the lo texels the tile's taps can touch (vr_tiles.h ScaledTileWindow: 12 x 12 at most, for F = 2) as records of three float4 -- the layer and
// the two float4 of the lo guide, 48 B a texel, 6912 B of LDS at most -- once, one barrier; threads outside a ragged hi frame stage and wait with the others,
// and texels off the lo frame hold a record no tap reads (the lane code skips such taps by their coordinates).  Then a pixel reads the two float4 of its hi
// features, forms its guide and B_p (rays x rays environment lookups, none with the environment hidden), runs its 16 taps from LDS and writes out and L, one
// dwordx4 each.  VR_UPSAMPLE_GLOBAL_TAPS = 1 builds the form whose taps read the three float4 from global memory instead (no LDS, no barrier): measured, not
// shipped.  No atomics, no scratch.  DEMOD ("denoise_demodulate" = 1, vr_demod.h): a lo record's layer is divided by the divisor of its own guide
// once, when it is staged -- the record's three float4 are in the staging thread's registers then, so the window holds the demodulated layer at the same size and
// the 16 taps read it as they do today -- and the pixel's hi layer is multiplied by the divisor of its hi features, which it has loaded for its guide.
#ifndef VR_UPSAMPLE_GLOBAL_TAPS
#define VR_UPSAMPLE_GLOBAL_TAPS 0
#endif
struct UpsampleTexel { float4 L, ga, gb; };
template <int32_t F>
struct UpsampleWindowDev {
    const UpsampleTexel* win;          // the staged window
    ScaledTileWindow<F> window;
    __device__ __forceinline__ void tap(int32_t lx, int32_t ly, float L[4], float g[8]) const {
        const UpsampleTexel& t = win[window.at(lx, ly)];
        unpack4(t.L, L); unpack4(t.ga, g); unpack4(t.gb, g + 4);
    }
};
struct UpsampleGlobalDev {
    const float4* __restrict__ L;
    const float4* __restrict__ g;
    int32_t w;
    __device__ __forceinline__ void tap(int32_t lx, int32_t ly, float Lq[4], float gq[8]) const {
        const int32_t i = ly * w + lx;
        unpack4(L[i], Lq); unpack4(g[2 * i], gq); unpack4(g[2 * i + 1], gq + 4);
    }
};
template <int32_t F, bool DEMOD>
__global__ void __launch_bounds__(256)
upsample_kernel(const SceneParams P, const float4* __restrict__ lo_layer, const float4* __restrict__ lo_guide, int32_t w, int32_t h,
                const float4* __restrict__ hi_features, int32_t rays, const DenoiseSigma sg, float4* __restrict__ out, float4* __restrict__ L) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    const TilePixel q = wave_tiled_pixel((int32_t)blockIdx.x, threadIdx.x, W);
#if !VR_UPSAMPLE_GLOBAL_TAPS
    using Window = ScaledTileWindow<F>;
    __shared__ UpsampleTexel win[Window::kTexels];
    const Window window = Window::of((int32_t)blockIdx.x, W);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    stage_window(win, window, w, h, UpsampleTexel{ zero, zero, zero }, [&](int32_t i) {
        UpsampleTexel t{ lo_layer[i], lo_guide[2 * i], lo_guide[2 * i + 1] };
        if constexpr (DEMOD) {
            float lq[4], ak[4];
            unpack4(t.L, lq); unpack4(t.ga, ak);
            demod_tap(lq, ak);
            t.L = pack4(lq);
        }
        return t;
    });
#endif
    if (q.px >= W || q.py >= H) return;
    const int32_t i = q.py * W + q.px;
    float f[8], gp[8], B[4], l[4], o[4];
    unpack4(hi_features[2 * i], f); unpack4(hi_features[2 * i + 1], f + 4);
    denoise_guide(f, gp);
    const v3 b = resolve_background(P, q.px, q.py, rays);
    B[0] = b.x; B[1] = b.y; B[2] = b.z; B[3] = 0.0f;
#if VR_UPSAMPLE_GLOBAL_TAPS
    if constexpr (DEMOD) demod_upsample_pixel(DemodTaps<UpsampleGlobalDev>{ { lo_layer, lo_guide, w } }, w, h, F, q.px, q.py, gp, B, sg, l, o);
    else upsample_pixel(UpsampleGlobalDev{ lo_layer, lo_guide, w }, w, h, F, q.px, q.py, gp, B, sg, l, o);
#else
    if constexpr (DEMOD) demod_upsample_pixel(UpsampleWindowDev<F>{ win, window }, w, h, F, q.px, q.py, gp, B, sg, l, o);
    else upsample_pixel(UpsampleWindowDev<F>{ win, window }, w, h, F, q.px, q.py, gp, B, sg, l, o);
#endif
    out[i] = pack4(o);
    L[i] = pack4(l);
}
void launch_upsample(const SceneParams& P, const float* lo_layer, const float* lo_guide, int32_t w, int32_t h, int32_t f, const float* hi_features, int32_t rays,
                     const DenoiseSigma& sg, float* out, float* L, hipStream_t stream, bool demod) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    if (f < kUpsampleMinFactor || f > kUpsampleMaxFactor || W != f * w || H != f * h) throw std::invalid_argument("launch_upsample: the hi frame is not f times the lo frame, f in 2..4");
    if (w <= 0 || h <= 0 || rays < 1) return;
    const dim3 grid((unsigned)tile_count(W, H)), block(256);
#define VR_UPSAMPLE_LAUNCH(F) hipLaunchKernelGGL((demod ? upsample_kernel<F, true> : upsample_kernel<F, false>), grid, block, 0, stream, P, reinterpret_cast<const float4*>(lo_layer), reinterpret_cast<const float4*>(lo_guide), \
                                                 w, h, reinterpret_cast<const float4*>(hi_features), rays, sg, reinterpret_cast<float4*>(out), reinterpret_cast<float4*>(L))
    if (f == 2) VR_UPSAMPLE_LAUNCH(2); else if (f == 3) VR_UPSAMPLE_LAUNCH(3); else VR_UPSAMPLE_LAUNCH(4);
#undef VR_UPSAMPLE_LAUNCH
}

// Adaptive sampling (vr_adaptive.h): e_t of every listed tile.  One workgroup per listed tile; each lane forms e_p of its pixel (-inf outside
// the frame: the identity of the max), a wave64 max by xor shuffles, the four waves' maxima through LDS, and lane 0 writes the tile's value.
// Max is exact, so the order of the reduction does not matter.
__global__ void __launch_bounds__(256)
adaptive_error_kernel(const float4* __restrict__ fb, const float4* __restrict__ moments, const int32_t* __restrict__ tiles, const int32_t* __restrict__ counts,
                      int32_t W, int32_t H, float* __restrict__ out) {
    __shared__ float wave_max[4];
    const int32_t tile = tiles[blockIdx.x], n = counts[blockIdx.x];
    const TilePixel q = wave_tiled_pixel(tile, threadIdx.x, W);
    float e = -inf_();
    if (q.px < W && q.py < H) {
        const size_t i = (size_t)q.py * W + q.px;
        float mu[4], S[4];
        unpack4(fb[i], mu); unpack4(moments[i], S);
        e = adaptive_pixel_error(mu, S, n);
    }
    for (int32_t d = 32; d > 0; d >>= 1) e = adaptive_max(e, __shfl_xor(e, d, 64));
    if (q.lane == 0) wave_max[q.sub] = e;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = adaptive_max(adaptive_max(wave_max[0], wave_max[1]), adaptive_max(wave_max[2], wave_max[3]));
}
void launch_adaptive_error(const float* fb, const float* moments, const int32_t* tiles, const int32_t* counts, int32_t n_tiles, int32_t W, int32_t H, float* out,
                           hipStream_t stream) {
    if (n_tiles <= 0 || W <= 0 || H <= 0) return;
    hipLaunchKernelGGL(adaptive_error_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, reinterpret_cast<const float4*>(fb),
                       reinterpret_cast<const float4*>(moments), tiles, counts, W, H, out);
}

// ---------------------------------------------------------------------------------------------------
// tonemap.glsl:13-36
__device__ __forceinline__ float hable(float x) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}
__global__ void __launch_bounds__(256)
tonemap_kernel(float* __restrict__ fb, int32_t n, float exposure, float inv_gamma) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4* p = reinterpret_cast<float4*>(fb) + i;
    float4 c = *p;
    const float hw = hable(11.2f);
    c.x = sanitize(pow_(hable(exposure * c.x) / hw, inv_gamma));
    c.y = sanitize(pow_(hable(exposure * c.y) / hw, inv_gamma));
    c.z = sanitize(pow_(hable(exposure * c.z) / hw, inv_gamma));
    c.w = sanitize(c.w);
    *p = c;
}
void launch_tonemap(float* fb, int32_t w, int32_t h, float exposure, float gamma, hipStream_t stream) {
    const int32_t n = w * h;
    if (n <= 0) return;
    hipLaunchKernelGGL(tonemap_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fb, n, exposure, 1.0f / gamma);
}

// ---------------------------------------------------------------------------------------------------
// tile <-> frame copies for the sharded framebuffer
__global__ void __launch_bounds__(256)
pack_tiles_kernel(const float* __restrict__ fb, int32_t w, int32_t h, const int32_t* __restrict__ tiles, float* __restrict__ packed) {
    const TilePixel q = raster_in_tile_pixel(tiles[blockIdx.x], threadIdx.x, w);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q.px < w && q.py < h) c = reinterpret_cast<const float4*>(fb)[(size_t)q.py * w + q.px];
    reinterpret_cast<float4*>(packed)[(size_t)blockIdx.x * 256 + threadIdx.x] = c;
}
__global__ void __launch_bounds__(256)
unpack_tiles_kernel(const float* __restrict__ packed, const int32_t* __restrict__ tiles, float* __restrict__ fb, int32_t w, int32_t h) {
    const int32_t tile = tiles[blockIdx.x];
    if (tile < 0) return;             // padding entry
    const TilePixel q = raster_in_tile_pixel(tile, threadIdx.x, w);
    if (q.px < w && q.py < h)
        reinterpret_cast<float4*>(fb)[(size_t)q.py * w + q.px] = reinterpret_cast<const float4*>(packed)[(size_t)blockIdx.x * 256 + threadIdx.x];
}
void launch_pack_tiles(const float* fb, int32_t w, int32_t h, const int32_t* tiles, int32_t n_tiles, float* packed, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(pack_tiles_kernel, dim3(n_tiles), dim3(256), 0, stream, fb, w, h, tiles, packed);
}
void launch_unpack_tiles(const float* packed, const int32_t* tiles, int32_t n_tiles, float* fb, int32_t w, int32_t h, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(unpack_tiles_kernel, dim3(n_tiles), dim3(256), 0, stream, packed, tiles, fb, w, h);
}
// The same for the denoiser's guide buffers, three float4 planes per pixel in one kernel (vr_tiles.h guide_slot): the moments texel and the two
// float4 of the pixel's features.  One workgroup per tile slot, raster in the tile; a pixel is three dwordx4 loads and three dwordx4 stores, each
// plane of a slot one contiguous 4 KiB run.  Pixels outside the frame pack as zeros and are not written on unpack.
__global__ void __launch_bounds__(256)
pack_guides_kernel(const float4* __restrict__ moments, const float4* __restrict__ features, int32_t w, int32_t h, const int32_t* __restrict__ tiles,
                   float4* __restrict__ packed) {
    const TilePixel q = raster_in_tile_pixel(tiles[blockIdx.x], threadIdx.x, w);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f), fa = m, fb = m;
    if (q.px < w && q.py < h) {
        const size_t i = (size_t)q.py * w + q.px;
        m = moments[i];
        fa = features[2 * i];
        fb = features[2 * i + 1];
    }
    packed[guide_slot(blockIdx.x, 0u, threadIdx.x)] = m;
    packed[guide_slot(blockIdx.x, 1u, threadIdx.x)] = fa;
    packed[guide_slot(blockIdx.x, 2u, threadIdx.x)] = fb;
}
__global__ void __launch_bounds__(256)
unpack_guides_kernel(const float4* __restrict__ packed, const int32_t* __restrict__ tiles, float4* __restrict__ moments, float4* __restrict__ features,
                     int32_t w, int32_t h) {
    const int32_t tile = tiles[blockIdx.x];
    if (tile < 0) return;             // padding entry
    const TilePixel q = raster_in_tile_pixel(tile, threadIdx.x, w);
    if (q.px >= w || q.py >= h) return;
    const size_t i = (size_t)q.py * w + q.px;
    moments[i] = packed[guide_slot(blockIdx.x, 0u, threadIdx.x)];
    features[2 * i] = packed[guide_slot(blockIdx.x, 1u, threadIdx.x)];
    features[2 * i + 1] = packed[guide_slot(blockIdx.x, 2u, threadIdx.x)];
}
void launch_pack_guides(const float* moments, const float* features, int32_t w, int32_t h, const int32_t* tiles, int32_t n_tiles, float* packed, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(pack_guides_kernel, dim3(n_tiles), dim3(256), 0, stream, reinterpret_cast<const float4*>(moments),
                       reinterpret_cast<const float4*>(features), w, h, tiles, reinterpret_cast<float4*>(packed));
}
void launch_unpack_guides(const float* packed, const int32_t* tiles, int32_t n_tiles, float* moments, float* features, int32_t w, int32_t h, hipStream_t stream) {
    if (n_tiles <= 0) return;
    hipLaunchKernelGGL(unpack_guides_kernel, dim3(n_tiles), dim3(256), 0, stream, reinterpret_cast<const float4*>(packed), tiles,
                       reinterpret_cast<float4*>(moments), reinterpret_cast<float4*>(features), w, h);
}

}  // namespace vr
