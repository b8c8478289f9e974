// vr_launch.hip -- launch of the volume path tracer (gfx950): launch_pathtrace, launch_features and launch_features_expected.
//
// pathtrace_kernel (the hot path): the per-path code -- the reference's trace_path and everything it calls, restated as a state
// machine -- is in vr_trace.h, its scheduler (persistent wavefronts that pull work units of 8x8 pixels x 8 samples) in vr_pathtrace.h and
// its compiled variants in vr_pathtrace.hip; vr_variant.h chooses the instance, this file sizes the launch and launches it.
// Radiance per (pixel, sample) goes to a sample pool; accumulate_kernel folds it into the RGBA32F running mean in sample
// order, which makes the result bit-identical to the reference's one-dispatch-per-sample loop (renderer.cpp:138-140,
// pathtracer_brick.glsl:36).  MFMA is not used: there is no dense contraction on this path.
// The tiles of a launch that no camera ray can hit the volume's box from, and those whose rays cross the box but cannot reach a voxel with density (vr_sky_tiles.h:
// clear and see-through tiles), never enter that path: sky_kernel renders them, one thread per pixel, straight into the running mean.
//
// Also here: the integrators that run one thread per (pixel, sample) item -- direct volume rendering (common.glsl:571-591)
// and ray marching --, which fill the same sample pool, and the denoiser's feature pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>

#include "vr_device.h"
#include "vr_expected.h"
#include "vr_pathtrace.h"

namespace vr {

// INTEGRATOR 2 (direct volume rendering, dvr_sample) and 3 (trace_path with the ray-marching trackers, raymarch_path_sample): one thread per
// (pixel, sample) item in queue position order, same sample-pool layout as the path-tracing kernel
template <int INTEGRATOR>
__global__ void __launch_bounds__(256)
item_kernel(const SceneParams P, float* __restrict__ sbuf, const LaunchDesc D) {
    const uint32_t per_unit = (uint32_t)(D.spu * 64);
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t u = g / per_unit, item = g - u * per_unit;
    if (u >= D.n_units) return;
    const WorkUnit wu = make_unit(D, P.u.resolution[0], u, sbuf);
    if ((int32_t)item >= wu.n_items) return;
    const int32_t px = wu.px0 + (int32_t)(item & 7u), py = wu.py0 + (int32_t)((item >> 3) & 7u);
    if (px >= P.u.resolution[0] || py >= P.u.resolution[1]) return;
    float L[4];
    if (INTEGRATOR == 2) dvr_sample(P, px, py, wu.first_sample + (int32_t)(item >> 6), L);
    else raymarch_path_sample(P, px, py, wu.first_sample + (int32_t)(item >> 6), L);
    reinterpret_cast<float4*>(sbuf)[wu.base + item] = pack4(L);
}

// One sample folded into a pixel's running mean (pathtracer_brick.glsl:36; accumulate_sample's arithmetic, vr_trace.h) as sample number `current_sample` (1-based).
// MOMENTS (variance = 1): also into the per-channel second moments, Welford in the running-mean form, S_k = M2_k / k.  The one statement of the mean on the
// device: accumulate_kernel and sky_kernel both fold through it.
template <bool MOMENTS>
__device__ __forceinline__ void fold_sample(float acc[4], float S[4], const float L[4], int32_t current_sample) {
    const float a = 1.0f / (float)current_sample;
    for (int32_t c = 0; c < 4; ++c) {
        const float x = sanitize(L[c]);
        const float mu = acc[c], mu1 = mix_(mu, x, a);
        if (MOMENTS) S[c] = mix_(S[c], (x - mu) * (x - mu1), a);
        acc[c] = mu1;
    }
}

// Running mean over the samples of one launch, in sample order: one workgroup per listed tile (tiles == nullptr: all tiles), one thread per pixel, every
// sample folded by fold_sample.  MOMENTS: the second moments in a W*H*4 buffer beside the colour.
template <bool MOMENTS>
__global__ void __launch_bounds__(256)
accumulate_kernel(const float* __restrict__ sbuf, float* __restrict__ fb, float* __restrict__ moments, const int32_t* __restrict__ tiles, int32_t n_tiles,
                  int32_t W, int32_t H, int32_t first_sample, int32_t n_samples, int32_t spu) {
    const TilePixel q = wave_tiled_pixel(tiles ? tiles[blockIdx.x] : (int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    float4* texel = reinterpret_cast<float4*>(fb) + (size_t)q.py * W + q.px;
    float4* mtexel = MOMENTS ? reinterpret_cast<float4*>(moments) + (size_t)q.py * W + q.px : nullptr;
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, S[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (first_sample > 1) {
        unpack4(*texel, acc);
        if (MOMENTS) unpack4(*mtexel, S);
    }
    const float4* sb = reinterpret_cast<const float4*>(sbuf);
    for (int32_t k = 0; k < n_samples; ++k) {
        const int32_t chunk = k / spu, sl = k - chunk * spu;
        float L[4];
        unpack4(sb[pool_slot<size_t>((size_t)chunk, n_tiles, (size_t)blockIdx.x, (uint32_t)q.sub, spu, (size_t)sl, (uint32_t)q.lane)], L);
        fold_sample<MOMENTS>(acc, S, L, first_sample + k);
    }
    *texel = pack4(acc);
    if (MOMENTS) *mtexel = pack4(S);
}

// The clear tiles of a launch (vr_sky_tiles.h: no camera ray of theirs can hit the volume's box): one workgroup per listed tile, one thread per pixel, laid out
// like accumulate_kernel.  Every sample of the launch's window is a primary miss -- sky_sample (vr_trace.h), its seed from the launch's seed table where that
// covers the sample number, hashed otherwise -- and is folded into the running mean as it is made, in sample order: no scheduler, no sample pool, and the lanes
// of a wavefront fetch neighbouring texels of the environment.  Starts from the framebuffer's texel when first_sample > 1.
// A ray that does hit the box means the classifier called a tile clear that is not: the pixel stops there and the kernel sets kSkyHitStatus in the renderer's
// status word (RendererHIP::check_watchdog throws).  A tripwire for a bug, never a fallback.
// The list is [clear | see-through]: the workgroups from n_clear on serve SEE-THROUGH tiles (vr_sky_tiles.h: rays that cross the box without a voxel with density
// in tap reach), whose samples are the same sky_sample without the box test -- hit or miss, the sample is the sky's; there is no tripwire to set for them.
template <bool MOMENTS>
__global__ void __launch_bounds__(256)
sky_kernel(const SceneParams P, float* __restrict__ fb, float* __restrict__ moments, const int32_t* __restrict__ tiles, int32_t n_clear, int32_t first_sample,
           int32_t n_samples, const SeedTable seeds, uint32_t* __restrict__ status) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    const bool box_test = (int32_t)blockIdx.x < n_clear;                      // uniform over the workgroup
    const TilePixel q = wave_tiled_pixel(tiles[blockIdx.x], threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    float4* texel = reinterpret_cast<float4*>(fb) + (size_t)q.py * W + q.px;
    float4* mtexel = MOMENTS ? reinterpret_cast<float4*>(moments) + (size_t)q.py * W + q.px : nullptr;
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, S[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (first_sample > 1) {
        unpack4(*texel, acc);
        if (MOMENTS) unpack4(*mtexel, S);
    }
    bool hit = false;
    for (int32_t k = 0; k < n_samples; ++k) {
        const int32_t smp = first_sample + k;
        uint32_t seed;
        if (seeds.table != nullptr && smp - 1 < seeds.cap) seed = seeds.table[seed_table_index<uint32_t>((uint32_t)(smp - 1), seeds.n_tiles, (uint32_t)q.tile, (uint32_t)q.sub, (uint32_t)q.lane)];
        else seed = path_seed((uint32_t)P.u.seed, W, q.px, q.py, smp);
        float L[4];
        if (!sky_sample(P, q.px, q.py, seed, L, box_test)) { hit = true; break; }
        fold_sample<MOMENTS>(acc, S, L, smp);
    }
    *texel = pack4(acc);
    if (MOMENTS) *mtexel = pack4(S);
    if (hit) atomicOr(status, kSkyHitStatus);
}

// Denoiser features (vr_trace.h feature_pixel): one thread per pixel of the renderer's tiles (tiles == nullptr: all tiles), all `spp` samples in a loop,
// laid out like accumulate_kernel.
// out: W*H*8 floats.  The first segment of the DDA tracker only, so a few registers' worth of state: no scheduler, no sample pool.
template <bool TF>
__global__ void __launch_bounds__(256)
features_kernel(const SceneParams P, const int32_t* __restrict__ tiles, int32_t spp, float* __restrict__ out, uint32_t* __restrict__ status) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    const TilePixel q = wave_tiled_pixel(tiles ? tiles[blockIdx.x] : (int32_t)blockIdx.x, threadIdx.x, W);
    if (q.px >= W || q.py >= H) return;
    float f[8];
    if (!feature_pixel<TF>(P, q.px, q.py, spp, f)) atomicOr(status, kFeatureLostStatus);      // a sample over its step budget (vr_trace.h feature_sample)
    float4* o = reinterpret_cast<float4*>(out) + 2u * ((size_t)q.py * W + q.px);
    o[0] = pack4(f);
    o[1] = pack4(f + 4);
}
void launch_features(const SceneParams& P, const int32_t* tiles, int32_t n_tiles, int32_t spp, float* out, uint32_t* status, hipStream_t stream) {
    if (n_tiles <= 0 || spp <= 0) return;
    if (P.u.use_tf) hipLaunchKernelGGL(features_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, stream, P, tiles, spp, out, status);
    else hipLaunchKernelGGL(features_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, stream, P, tiles, spp, out, status);
}

// The same buffer filled with expected values instead of sample means (vr_expected.h expected_pixel): one thread per pixel on the same tiles, rays x rays
// deterministic marches of at most kExpectedMaxSteps steps each -- a bounded loop, so no status word.  An 8x8 patch of neighbouring rays walks the same bricks
// nearly in lockstep: a step's eight corner taps mostly hit lines a neighbouring lane has just loaded, and trip counts differ only at silhouettes.  The LUT is read
// from global memory: its two rows per step are shared by neighbouring lanes too, and the kernel keeps its registers and LDS for occupancy.
// SKIP: the instance that reads the clear-distance table `clear` (vr_expected.h: steps in clear cells are dropped with their loads, same bits); the table is an
// argument of this kernel alone.  STATS: the instrumented twin: every lane counts (ExpectedWork), the wavefront sums, and its lanes 0..3 add one total each to
// stats[0..3] in one atomic instruction.  No lane leaves before that sum.
// CUBIC (without a LUT only): the instances that march the tracker's cubic B-spline field (vr_cubic.h: 64 taps a step in at most 2 x 2 x 2 cells, whose indices and
// decode ranges are formed once per step); `clear` is then the table of reach 2.
template <bool TF, bool SKIP, bool STATS, bool CUBIC = false>
__global__ void __launch_bounds__(256)
features_expected_kernel(const SceneParams P, const int32_t* __restrict__ tiles, int32_t rays, float* __restrict__ out, const ClearTable clear,
                         unsigned long long* __restrict__ stats) {
    const int32_t W = P.u.resolution[0], H = P.u.resolution[1];
    const TilePixel q = wave_tiled_pixel(tiles ? tiles[blockIdx.x] : (int32_t)blockIdx.x, threadIdx.x, W);
    const bool live = q.px < W && q.py < H;
    if (!STATS && !live) return;
    ExpectedWork work = { 0u, 0u, 0u, 0u, 0u };
    if (live) {
        float f[8];
        expected_pixel<TF, false, SKIP, STATS, false, CUBIC>(P, q.px, q.py, rays, f, nullptr, SKIP ? &clear : nullptr, STATS ? &work : nullptr);
        float4* o = reinterpret_cast<float4*>(out) + 2u * ((size_t)q.py * W + q.px);
        o[0] = pack4(f);
        o[1] = pack4(f + 4);
    }
    if (STATS) {
        uint32_t v[4] = { work.rays, work.steps, work.fetched, work.reads };      // per lane at most 16 x 4096 steps: the sums of 64 lanes fit
#pragma unroll
        for (int c = 0; c < 4; ++c)
            for (int o = 32; o > 0; o >>= 1) v[c] += (uint32_t)__shfl_xor((int)v[c], o);
        const uint32_t lane = threadIdx.x & 63u;
        if (lane < 4u) atomicAdd(stats + lane, (unsigned long long)(lane == 0u ? v[0] : (lane == 1u ? v[1] : (lane == 2u ? v[2] : v[3]))));
    }
}
void launch_features_expected(const SceneParams& P, const int32_t* tiles, int32_t n_tiles, int32_t rays, float* out, hipStream_t stream,
                              const ClearTable* clear, unsigned long long* stats, bool cubic) {
    if (n_tiles <= 0 || rays < 1 || rays > kExpectedMaxRays) return;
    const bool skip = clear && clear->d;
    const ClearTable C = skip ? *clear : ClearTable{ nullptr, { 0, 0, 0 } };
    const bool tf = P.u.use_tf != 0;
    const dim3 grid((unsigned)n_tiles), block(256);
#define VR_EXPECTED_LAUNCH(TF, SKIP, STATS) hipLaunchKernelGGL((features_expected_kernel<TF, SKIP, STATS>), grid, block, 0, stream, P, tiles, rays, out, C, stats)
    if (cubic && !tf) {                             // under a LUT the tracker's field is the trilinear one: the instances below
#define VR_EXPECTED_CUBIC(SKIP, STATS) hipLaunchKernelGGL((features_expected_kernel<false, SKIP, STATS, true>), grid, block, 0, stream, P, tiles, rays, out, C, stats)
        if (stats) { if (skip) VR_EXPECTED_CUBIC(true, true); else VR_EXPECTED_CUBIC(false, true); }
        else { if (skip) VR_EXPECTED_CUBIC(true, false); else VR_EXPECTED_CUBIC(false, false); }
#undef VR_EXPECTED_CUBIC
    } else if (stats) {
        if (skip) { if (tf) VR_EXPECTED_LAUNCH(true, true, true); else VR_EXPECTED_LAUNCH(false, true, true); }
        else { if (tf) VR_EXPECTED_LAUNCH(true, false, true); else VR_EXPECTED_LAUNCH(false, false, true); }
    } else {
        if (skip) { if (tf) VR_EXPECTED_LAUNCH(true, true, false); else VR_EXPECTED_LAUNCH(false, true, false); }
        else { if (tf) VR_EXPECTED_LAUNCH(true, false, false); else VR_EXPECTED_LAUNCH(false, false, false); }
    }
#undef VR_EXPECTED_LAUNCH
}

// samples of a work unit: the tuning's, or the variant's own (vr_variant.h)
static int32_t samples_per_unit(const PathtraceTuning& T, int32_t variant_default) { return T.samples_per_unit > 0 ? T.samples_per_unit : variant_default; }

PathtraceTuning default_tuning() {
    static std::once_flag once;
    static int32_t env_spu = 0, env_blocks = 0;       // diagnostics only
    std::call_once(once, [] {
        if (const char* e = getenv("VR_SPU")) env_spu = std::max(1, atoi(e));
        if (const char* e = getenv("VR_BLOCKS_PER_CU")) env_blocks = std::max(0, atoi(e));
    });
    PathtraceTuning T;
    T.samples_per_unit = env_spu;
    T.blocks_per_cu = env_blocks;
    return T;
}

size_t pathtrace_pool_floats(const PathtraceTuning& T, int32_t n_tiles, int32_t n_samples) {
    // the samples are rounded up to whole units: sized for whichever unit size a variant may use (samples_per_unit)
    size_t padded = 0;
    for (int variant = 0; variant < kPtVariants; ++variant) {
        const int32_t spu = std::min(n_samples, samples_per_unit(T, pathtrace_unit_samples(variant)));
        padded = std::max(padded, (size_t)((n_samples + spu - 1) / spu) * (size_t)spu);
    }
    return padded * (size_t)n_tiles * 4u * 64u * 4u;
}

// the kernel variants live in vr_pathtrace.hip, one compilation each, in two arithmetic modes (bit-exact / tolerance)
extern "C" {
#define VR_PT_DECL(N) \
    int vr_pt_occupancy_##N(int tf, int stats); \
    void vr_pt_launch_##N(int tf, int stats, unsigned grid, hipStream_t stream, const void* P, float* sbuf, float* cold_ws, const void* D, const void* S, uint32_t* status, unsigned long long* stats_buf, const void* seeds);
VR_PT_DECL(0) VR_PT_DECL(1) VR_PT_DECL(2) VR_PT_DECL(3) VR_PT_DECL(4) VR_PT_DECL(0_fast) VR_PT_DECL(1_fast) VR_PT_DECL(2_fast) VR_PT_DECL(3_fast) VR_PT_DECL(4_fast)
VR_PT_DECL(0w) VR_PT_DECL(1w) VR_PT_DECL(0w_fast) VR_PT_DECL(1w_fast)      // 64-bit gather addresses (VR_PT_WIDE)
#undef VR_PT_DECL
}
typedef int (*PtOccupancy)(int, int);
typedef void (*PtLaunch)(int, int, unsigned, hipStream_t, const void*, float*, float*, const void*, const void*, uint32_t*, unsigned long long*, const void*);
// [arithmetic mode][instance], in the order of vr_variant.h PathtraceKernel::instance
static const struct { PtOccupancy occupancy; PtLaunch launch; } kPtInstance[2][kPtInstances] = {
    { { vr_pt_occupancy_0, vr_pt_launch_0 }, { vr_pt_occupancy_0w, vr_pt_launch_0w }, { vr_pt_occupancy_1, vr_pt_launch_1 }, { vr_pt_occupancy_1w, vr_pt_launch_1w },
      { vr_pt_occupancy_2, vr_pt_launch_2 }, { vr_pt_occupancy_4, vr_pt_launch_4 }, { vr_pt_occupancy_3, vr_pt_launch_3 } },
    { { vr_pt_occupancy_0_fast, vr_pt_launch_0_fast }, { vr_pt_occupancy_0w_fast, vr_pt_launch_0w_fast }, { vr_pt_occupancy_1_fast, vr_pt_launch_1_fast }, { vr_pt_occupancy_1w_fast, vr_pt_launch_1w_fast },
      { vr_pt_occupancy_2_fast, vr_pt_launch_2_fast }, { vr_pt_occupancy_4_fast, vr_pt_launch_4_fast }, { vr_pt_occupancy_3_fast, vr_pt_launch_3_fast } } };

// The run-time variant (3) is an order of magnitude slower than the kernels of one scene kind on some scenes (one copy of the hot pair, general forms only, everything
// decided per wavefront), so a scene that lands there for a reason its caller did not ask for is told so (here, and vr_get_int "kernel_variant_reason").
// The two reasons a caller cannot see coming: said once per process, on stderr
static void note_unexpected_reasons(int why) {
    if (why & (VR_VARIANT_ENV_DIVISION | VR_VARIANT_DENSITY_SCALE)) {
        static std::once_flag once;
        std::call_once(once, [&] {
            fprintf(stderr, "volren_amd: note: this scene is rendered by the run-time kernel variant (slower; results unchanged):%s%s\n",
                    (why & VR_VARIANT_ENV_DIVISION) ? " the environment's warp table has thresholds below 2^-76 (vr_get_int env_div_safe = 0);" : "",
                    (why & VR_VARIANT_DENSITY_SCALE) ? " the density scale lies outside [2^-16, 2^24];" : "");
        });
    }
}

// resident workgroups of a kernel instance on the CURRENT device: occupancy query x CU count, cached per (device, instance)
static int resident_blocks(const PathtraceTuning& T, int mode, int instance, bool tf, bool stats) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1024;
    static std::mutex mu;
    static std::map<uint32_t, std::pair<int, int>> cache;            // key -> (CUs, workgroups per CU)
    const uint32_t key = ((uint32_t)dev << 8) | ((uint32_t)mode << 5) | ((uint32_t)instance << 2) | (tf ? 2u : 0u) | (stats ? 1u : 0u);
    std::pair<int, int> v;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = cache.find(key);
        if (it == cache.end()) {
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
            it = cache.emplace(key, std::make_pair(cus, kPtInstance[mode][instance].occupancy(tf, stats))).first;
        }
        v = it->second;
    }
    const int per_cu = T.blocks_per_cu > 0 ? T.blocks_per_cu : v.second;
    return std::min(v.first * per_cu, kMaxWorkgroups * 4 / kWgWaves);
}

size_t pathtrace_workspace_floats() { return kColdMainFloats + (size_t)kMaxWorkgroups * 4u * (size_t)kColdSideWaveFloats; }      // cold state of 4 wavefronts per resident workgroup: main slots, then the side array

void launch_pathtrace(const PathtraceTuning& T, const SceneParams& P, float* fb, float* sample_pool, float* workspace, uint32_t* unit_counter, const int32_t* tiles, int32_t n_tiles,
                      int32_t first_sample, int32_t n_samples, uint32_t* status, hipStream_t stream, bool fast_math, hipEvent_t ev_kernel_begin, hipEvent_t ev_kernel_end,
                      float* moments, const uint32_t* seed_table, int32_t seed_samples, const int32_t* sky_tiles, int32_t n_sky_tiles, int32_t n_see_tiles) {
    if (n_samples <= 0 || (n_tiles <= 0 && n_sky_tiles + n_see_tiles <= 0)) return;
    SeedTable seeds;
    seeds.table = seed_samples > 0 ? seed_table : nullptr;
    seeds.cap = seed_samples;
    seeds.n_tiles = tile_count(P.u.resolution[0], P.u.resolution[1]);
    // the clear and the see-through tiles of the launch, in one launch behind the path-tracing kernel on the same stream and inside the same pair of events
    auto launch_sky = [&] {
        if (n_sky_tiles + n_see_tiles <= 0) return;
        const auto sky = moments ? sky_kernel<true> : sky_kernel<false>;
        hipLaunchKernelGGL(sky, dim3((unsigned)(n_sky_tiles + n_see_tiles)), dim3(256), 0, stream, P, fb, moments, sky_tiles, n_sky_tiles, first_sample, n_samples, seeds, status);
    };
    if (n_tiles <= 0) {                             // every tile of the launch is clear or see-through: no path-tracing kernel, no sample pool
        if (ev_kernel_begin) (void)hipEventRecord(ev_kernel_begin, stream);
        launch_sky();
        if (ev_kernel_end) (void)hipEventRecord(ev_kernel_end, stream);
        return;
    }
    SchedParams S;
    for (int i = 0; i < ST_COUNT; ++i) S.thr[i] = T.thr[i];
    LaunchDesc D;
    D.tiles = tiles; D.n_tiles = n_tiles; D.first_sample = first_sample; D.n_samples = n_samples;
    const bool tf = P.u.use_tf != 0, stats = T.stats != nullptr;
    const PathtraceKernel K = pathtrace_kernel_of(P, T.wide_addressing != 0, stats);
    note_unexpected_reasons(K.reason);
    D.spu = std::min(n_samples, samples_per_unit(T, K.samples_per_unit));
    const int32_t chunks = (n_samples + D.spu - 1) / D.spu;
    // item indices are 32-bit (WorkUnit::base, the sample pool's slots): RendererHIP::samples_per_launch sizes sub-launches below that; anything else is a caller's bug
    if ((uint64_t)chunks * (uint64_t)n_tiles * 4u * (uint64_t)(D.spu * 64) > 0xFFFFFFFFull)
        throw std::runtime_error("launch_pathtrace: " + std::to_string(n_tiles) + " tiles x " + std::to_string(n_samples) + " samples do not fit the 32-bit item index of one launch");
    D.n_units = (uint32_t)chunks * (uint32_t)n_tiles * 4u;
    D.chunks = (uint32_t)chunks;
    D.seg_len = (D.n_units + kQueueSegments - 1u) / kQueueSegments;
    D.unit_counter = unit_counter;
    S.max_iters = kMaxIdleIters;
    // lanes that must stand at a tentative collision before the collision code runs while others still march (vr_pathtrace.h):
    // measured optimum 24 (smoke.brick +0.5 %, dense +0.7 %, sparse + emission +2...3.5 %), 32 with a transfer function, whose
    // collision code (8 corner taps + LUT) is the dearest (+4.4 %); profiles/r2ab_collide_threshold.txt
    // (round 4: 32 also with an emission grid, whose collision code carries two stochastic taps: c5cloud +0.8 %, c5full +1 %, profiles/r4a_*)
    if (S.thr[ST_COLLIDE] <= 0) S.thr[ST_COLLIDE] = (P.u.use_tf || P.u.has_emission) ? 32 : 24;
    const int mode = fast_math ? 1 : 0;
    const int blocks = resident_blocks(T, mode, K.instance, tf, stats);
    const uint32_t groups_needed = (D.n_units + (uint32_t)kWgWaves - 1u) / (uint32_t)kWgWaves;      // a wavefront per unit at least
    const dim3 grid((unsigned)std::min<uint32_t>((uint32_t)blocks, groups_needed > 0 ? groups_needed : 1u)), block(256);
    if (K.item_integrator) {
        const uint64_t items = (uint64_t)D.n_units * (uint64_t)(D.spu * 64);
        const auto integrate = K.item_integrator == 2 ? item_kernel<2> : item_kernel<3>;
        hipLaunchKernelGGL(integrate, dim3((unsigned)((items + 255) / 256)), block, 0, stream, P, sample_pool, D);
        launch_sky();                               // (the renderer splits no launch of these integrators)
    } else {
        (void)hipMemsetAsync(unit_counter, 0, kQueueSegments * sizeof(uint32_t), stream);
        if (ev_kernel_begin) (void)hipEventRecord(ev_kernel_begin, stream);
        kPtInstance[mode][K.instance].launch(tf, stats, grid.x, stream, &P, sample_pool, workspace, &D, &S, status, T.stats, &seeds);
        launch_sky();
        if (ev_kernel_end) (void)hipEventRecord(ev_kernel_end, stream);
    }
    const auto accumulate = moments ? accumulate_kernel<true> : accumulate_kernel<false>;
    hipLaunchKernelGGL(accumulate, dim3((unsigned)n_tiles), block, 0, stream, sample_pool, fb, moments, tiles, n_tiles, P.u.resolution[0], P.u.resolution[1],
                       first_sample, n_samples, D.spu);
}

}  // namespace vr
