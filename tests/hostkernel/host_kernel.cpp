// tests/hostkernel/host_kernel.cpp -- TEST HARNESS ONLY, never part of the product.
//
// Compiles the device code of the path tracer (volren_amd/csrc/vr_trace.h, vr_math.h -- the same headers the HIP
// kernel is built from) with the host compiler so that the lane state machine can be checked against the CPU
// oracle, and run under ASan/UBSan, in the GPU-less build container.  It is built and loaded by
// tests/test_host_kernel.py only; the product library (libvolren_amd.so) has no CPU path.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../volren_amd/csrc/vr_variant.h"
#include "../../volren_amd/csrc/vr_tiles.h"
#include "host_scene.h"

using namespace vr;
using namespace hostscene;


// ---- access trace (tests/tools_coherence_by_scope.py): which 128-byte line of the majorant table a marching path's next DDA step reads, which
// 4x4x4-voxel block (one line of the dense grid) / 8^3 brick a path at a tentative collision stands in.  One 32-bit word per lane-step:
// bits 31..30 = 0 march / 1 collide, bits 29..0 = line id.  Test infrastructure only.
static uint32_t* g_trace = nullptr;
static size_t g_trace_cap = 0, g_trace_n = 0;
static void trace_access(const Hot& h, const SceneParams& P) {
    if (g_trace_n >= g_trace_cap) return;
    const v3 c = axpy(h.ipos, h.t, h.idir);
    if (h.state == ST_MARCH) {
        if (!(h.t < seg_far(h))) return;                                               // (the sign of `far` carries the clean flag: vr_trace.h seg_clean)
        const int32_t idx = majorant_index<2>(P.density, c, round_mip_q(h.mipq));
        if (idx >= 0 && idx != P.density.maj_outside) g_trace[g_trace_n++] = (uint32_t)idx >> 6;      // 64 fp16 cells per 128-byte line; a step outside the table reads its one shared "outside" cell: not a gather
    } else {
        const int32_t x = (int32_t)floor_(c.x), y = (int32_t)floor_(c.y), z = (int32_t)floor_(c.z);
        if (x < 0 || y < 0 || z < 0) return;
        const uint32_t sh = P.density.dense ? 2u : 3u;                                  // dense: 4x4x4 block = one line; bricks: 8^3 block = 4 lines
        const uint32_t nx = P.density.dense ? (uint32_t)P.density.dblk[0] : (uint32_t)P.density.nb[0], ny = P.density.dense ? (uint32_t)P.density.dblk[1] : (uint32_t)P.density.nb[1];
        const uint32_t id = (((uint32_t)z >> sh) * ny + ((uint32_t)y >> sh)) * nx + ((uint32_t)x >> sh);
        g_trace[g_trace_n++] = (1u << 30) | (id & 0x3FFFFFFFu);
    }
}

// ---- the compiled forms of the lane code: exactly the 14 configurations the device ships (volren_amd/csrc/vr_pathtrace.hip Cfg) -----------------------------------
// form = 2 * slot + (transfer function ? 1 : 0); slots = the product's instances (vr_variant.h PathtraceKernel::instance): 0 variant 0 with 32-bit gather offsets, 1 variant 0 with 64-bit addresses ("wide"), 2 and 3 the same for variant 1,
// 4 variant 2, 5 variant 4, 6 variant 3 (the last three always form 64-bit addresses).  What stays out is what only the device's scheduler has: the emission
// state cached in the hot registers (collide_finish's CACHED) and the LDS stores.
enum { HK_SLOTS = 7, HK_FORMS = 2 * HK_SLOTS, HK_COUNTERS = 18 };
template <int SLOT, bool TF> struct FormCfg;
template <bool TF> struct FormCfg<0, TF> { using type = TraceCfg<TF, 0, 0, 0, 0, true>; };
template <bool TF> struct FormCfg<1, TF> { using type = TraceCfg<TF, 0, 0, 0, 0, false>; };
template <bool TF> struct FormCfg<2, TF> { using type = TraceCfg<TF, 0, 0, 1, 0, true>; };
template <bool TF> struct FormCfg<3, TF> { using type = TraceCfg<TF, 0, 0, 1, 0, false>; };
template <bool TF> struct FormCfg<4, TF> { using type = TraceCfg<TF, 0, 1, 0, 0, false>; };
template <bool TF> struct FormCfg<5, TF> { using type = TraceCfg<TF, 0, 1, 0, 1, false>; };
template <bool TF> struct FormCfg<6, TF> { using type = TraceCfg<TF, 2, 2, 2, 2, false>; };
// per form since the last hk_form_steps(reset): [0] lane steps, then the steps of the hot pair by the segment's kind, counted before each lane_step from seg_clean(l)
// and l.state: [1] march on a clean segment, [2] collide on a clean one, [3] march on a segment that is not clean (the general forms), [4] collide on such a one.
// Then what the device scheduler's instrumented instances count per block (vr_pathtrace.h VR_STAT: the lanes a block ran for), here per path and so whatever the
// scheduler: lane steps by the state they were ENTERED in, counted before the step -- [5] NEW (only a step that takes an item: the harness's own last step of a
// lane, NEW -> DONE, is no item), [6] MARCH (one pass of up to two DDA iterations, as on the device), [7] COLLIDE, [8] NEE, [9] POSTNEE, [10] ESCAPE -- and the
// transitions that end a path or an item, counted after it: [11] POSTNEE -> NEW (bounce cap or roulette), [12] NEW -> NEW (the item's pixel lies outside a ragged
// frame), [13] NEW -> ESCAPE (the camera segment ends before it begins), [14] those of [13] whose camera ray misses the volume's box (the others, global-majorant
// trackers only, hit it and draw a free flight beyond it).  [15] the DDA iterations the march passes of [6] went through and [16] the passes among them that went
// through none (entered with t >= far), both read off march_prep / march_load as march_finish reads them; [17] NEE steps that start a shadow segment
enum { HC_NEW = 5, HC_MARCH, HC_COLLIDE, HC_NEE, HC_POSTNEE, HC_ESCAPE, HC_ENDED, HC_OUTSIDE, HC_NEW_ESCAPE, HC_PRIMARY_MISS, HC_DDA, HC_MARCH_EMPTY, HC_SHADOW };
static unsigned long long g_form_steps[HK_FORMS][HK_COUNTERS] = {};

struct ColdHost {
    float v[C_COUNT];
    float ld(int32_t f) const { return v[f]; }
    void st(int32_t f, float x) { v[f] = x; }
};

// The scene with the views the serving kernel gets (RendererHIP::fill_params): two brick grids that can share a paired atlas, in a scene nothing sends to the
// run-time variant (vr_variant.h), are read from ONE paired atlas -- and only that kernel reads a majorant table whose levels 0-1 are in 4x4x4-cell blocks; for
// every other scene the table is built linear, whatever the caller asked for.
static void build_lane_scene(HostScene& S, const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                             const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int flags) {
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim, flags);
    SceneParams& P = S.P;
    const bool paired = scene_pairs_atlases(P);      // (has_emission without an emission descriptor: the emission view stays as HostScene value-initialised it, all zeros, which pairs with no grid)
    if (!paired && P.density.maj_blocked) build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim, flags | HS_MAJ_LINEAR);
    if (paired) {
        build_paired_atlas(S.dg, S.eg, S.paired);
        P.density.atlas = S.paired.data();
        P.emission.atlas = S.paired.data();
        P.paired = 1;
    }
}

// DDA iterations of the march pass lane_step is about to run for `l` (0, 1 or 2): march_finish's own tests on march_prep's and march_load's values
template <class K>
static int march_pass_iterations(const Hot& l, const SceneParams& P) {
    MarchIO io;
    if (seg_clean(l)) march_prep<K::dense, K::majb, true>(l, P, io); else march_prep<K::dense, K::majb, false>(l, P, io);
    if (!io.go1) return 0;
    march_load<K::tf, K::a32>(P, io);
    const float tau = l.tau - majorant_value<K::tf>(P, io.maj1) * io.dt1;
    return (tau > 0.0f && io.go2) ? 2 : 1;
}

// one work unit on 64 lanes advanced round-robin: exercises the item hand-out in a different order than the GPU does
template <class K>
static bool run_unit(const SceneParams& P, unsigned long long* count, const WorkUnit& wu, long long& steps) {
    Hot lanes[64];
    ColdHost cold[64] = {};
    FirstStash stash[64] = {};
    for (auto& l : lanes) hot_init(l);
    uint32_t next_item = 0;
    bool live = true;
    while (live) {
        live = false;
        for (int i = 0; i < 64; ++i) {
            Hot& l = lanes[i];
            if (l.state == ST_DONE) continue;
            live = true;
            if (l.state == ST_NEW) for (float& v : cold[i].v) v = nan_();         // a new path must not depend on what its cold line held
            if (l.state == ST_MARCH || l.state == ST_COLLIDE) {
                if (g_trace) trace_access(l, P);
                ++count[(seg_clean(l) ? 1 : 3) + (l.state == ST_COLLIDE ? 1 : 0)];
            }
            const int32_t st = l.state;
            if (st == ST_MARCH) { const int it = march_pass_iterations<K>(l, P); count[HC_DDA] += (unsigned)it; if (it == 0) ++count[HC_MARCH_EMPTY]; }
            const bool took_item = st == ST_NEW && next_item < (uint32_t)wu.n_items;
            if (took_item) ++count[HC_NEW];
            else if (st >= ST_MARCH && st <= ST_ESCAPE) ++count[HC_MARCH + (st - ST_MARCH)];
            lane_step<K>(l, cold[i], P, wu, next_item, stash[i]);
            if (st == ST_POSTNEE && l.state == ST_NEW) ++count[HC_ENDED];
            if (took_item && l.state == ST_NEW) ++count[HC_OUTSIDE];
            if (took_item && l.state == ST_ESCAPE) {
                ++count[HC_NEW_ESCAPE];
                // a ray that misses the box leaves a `first` path (do_new), whose direction is in the stash; the box test is begin_segment's
                float tn, tf;
                if (l.first && !intersect_box(v3{ P.u.cam_pos[0], P.u.cam_pos[1], P.u.cam_pos[2] }, stash[i].dir, P.u.vol_bb_min, P.u.vol_bb_max, tn, tf)) ++count[HC_PRIMARY_MISS];
            }
            if (st == ST_NEE && l.shadow) ++count[HC_SHADOW];
            ++count[0];
            if (++steps > (1ll << 40)) return false;
        }
    }
    return true;
}

// wave-sized work units exactly like the HIP kernel: 8x8 tile x chunk of samples -> sample buffer -> running mean
template <class K>
static long long render_units(const SceneParams& P, int form, float* fb, int x0, int y0, int x1, int y1, int first_sample, int n_samples) {
    const Uniforms& u = P.u;
    const int W = u.resolution[0], H = u.resolution[1];
    long long steps = 0;
    unsigned long long* count = g_form_steps[form];
    const int spu = n_samples < 32 ? n_samples : 32;
    std::vector<float> sbuf((size_t)spu * 64 * 4);
    for (int ty = y0 & ~7; ty < y1; ty += 8)
        for (int tx = x0 & ~7; tx < x1; tx += 8)
            for (int c0 = 0; c0 < n_samples; c0 += spu) {
                WorkUnit wu;
                wu.px0 = tx; wu.py0 = ty; wu.first_sample = first_sample + c0;
                const int sc = (n_samples - c0) < spu ? (n_samples - c0) : spu;
                wu.n_items = sc * 64; wu.base = 0u; wu.out = sbuf.data();
                if (!run_unit<K>(P, count, wu, steps)) return -1;
                for (int p = 0; p < 64; ++p) {
                    const int x = tx + (p & 7), y = ty + (p >> 3);
                    if (x < x0 || x >= x1 || y < y0 || y >= y1 || x >= W || y >= H) continue;
                    float* px = fb + 4 * ((size_t)y * W + x);
                    for (int k = 0; k < sc; ++k) accumulate_sample(px, &sbuf[4 * ((size_t)k * 64 + p)], first_sample + c0 + k);
                }
            }
    return steps;
}

// The device's items for a tile list (vr_pathtrace.h make_unit): every listed 16x16 tile's four 8x8 sub-tiles, each in chunks of `spu` samples, 64 items per sample
// -- the items whose pixel lies outside a ragged frame included, as the device's NEW batches take them (tiles == nullptr: tiles 0 .. n_tiles - 1)
template <class K>
static long long render_tiles(const SceneParams& P, int form, float* fb, const int32_t* tiles, int n_tiles, int first_sample, int n_samples, int spu) {
    const Uniforms& u = P.u;
    const int W = u.resolution[0], H = u.resolution[1];
    long long steps = 0;
    unsigned long long* count = g_form_steps[form];
    if (spu > n_samples) spu = n_samples;
    std::vector<float> sbuf((size_t)spu * 64 * 4);
    for (int slot = 0; slot < n_tiles; ++slot)
        for (uint32_t sub = 0; sub < 4u; ++sub)
            for (int c0 = 0; c0 < n_samples; c0 += spu) {
                const TilePixel q = wave_tiled_pixel(tiles ? tiles[slot] : slot, sub * 64u, W);
                WorkUnit wu;
                wu.px0 = q.px; wu.py0 = q.py; wu.first_sample = first_sample + c0;
                const int sc = (n_samples - c0) < spu ? (n_samples - c0) : spu;
                wu.n_items = sc * 64; wu.base = 0u; wu.out = sbuf.data();
                if (!run_unit<K>(P, count, wu, steps)) return -1;
                for (int p = 0; p < 64; ++p) {
                    const int x = q.px + (p & 7), y = q.py + (p >> 3);
                    if (x >= W || y >= H) continue;
                    float* px = fb + 4 * ((size_t)y * W + x);
                    for (int k = 0; k < sc; ++k) accumulate_sample(px, &sbuf[4 * ((size_t)k * 64 + p)], first_sample + c0 + k);
                }
            }
    return steps;
}

extern "C" {

int hk_uniforms_size() { return (int)sizeof(Uniforms); }
int hk_form_count() { return HK_FORMS; }
void hk_form_steps(unsigned long long out[HK_FORMS * HK_COUNTERS], int reset) {
    for (int f = 0; f < HK_FORMS; ++f) for (int k = 0; k < HK_COUNTERS; ++k) { if (out) out[f * HK_COUNTERS + k] = g_form_steps[f][k]; if (reset) g_form_steps[f][k] = 0; }
}

// env_rgb: texture order (row 0 bottom), 3 floats per texel.  force_wide: the 64-bit form of variants 0 and 1 whatever the tables' sizes (the product's
// "wide_addressing"); flags: host_scene.h HS_*.  Returns the number of lane steps executed.
long long hk_render(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                    const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim,
                    float* fb, int x0, int y0, int x1, int y1, int first_sample, int n_samples, int force_wide, int flags) {
    HostScene S;
    build_lane_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim, flags);
    const SceneParams& P = S.P;
    const Uniforms& u = P.u;
    const PathtraceKernel kernel = pathtrace_kernel_of(P, force_wide != 0, false);      // the product's own rule (vr_variant.h)
    long long steps = 0;
    const int W = u.resolution[0];
    if (kernel.item_integrator == 2) {         // direct volume rendering: one call per (pixel, sample)
        for (int y = y0; y < y1; ++y) for (int x = x0; x < x1; ++x) {
            float* px = fb + 4 * ((size_t)y * W + x);
            for (int k = 0; k < n_samples; ++k) { float L[4]; dvr_sample(P, x, y, first_sample + k, L); accumulate_sample(px, L, first_sample + k); ++steps; }
        }
        return steps;
    }
    if (kernel.item_integrator == 3) {         // trace_path with the ray-marching trackers: one call per (pixel, sample)
        for (int y = y0; y < y1; ++y) for (int x = x0; x < x1; ++x) {
            float* px = fb + 4 * ((size_t)y * W + x);
            for (int k = 0; k < n_samples; ++k) { float L[4]; raymarch_path_sample(P, x, y, first_sample + k, L); accumulate_sample(px, L, first_sample + k); ++steps; }
        }
        return steps;
    }
    const int form = 2 * kernel.instance + (u.use_tf ? 1 : 0);
    switch (form) {
#define HK_FORM(SLOT) \
    case 2 * SLOT: return render_units<FormCfg<SLOT, false>::type>(P, form, fb, x0, y0, x1, y1, first_sample, n_samples); \
    case 2 * SLOT + 1: return render_units<FormCfg<SLOT, true>::type>(P, form, fb, x0, y0, x1, y1, first_sample, n_samples);
    HK_FORM(0) HK_FORM(1) HK_FORM(2) HK_FORM(3) HK_FORM(4) HK_FORM(5) HK_FORM(6)
#undef HK_FORM
    default: return -1;
    }
}

// The same scene and form rule, walked as the device walks a launch: the items of the `n_tiles` listed 16x16 tiles (raster ids, row 0 = bottom; tiles == nullptr:
// every tile of the frame), in work units of the serving kernel's own size.  Path-tracing forms only (-2 for the item integrators, which have no scheduler).
long long hk_render_tiles(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                          const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim,
                          float* fb, const int32_t* tiles, int n_tiles, int first_sample, int n_samples, int force_wide, int flags) {
    HostScene S;
    build_lane_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim, flags);
    const SceneParams& P = S.P;
    const PathtraceKernel kernel = pathtrace_kernel_of(P, force_wide != 0, false);
    if (kernel.item_integrator != 0) return -2;
    if (n_samples <= 0) return 0;
    if (!tiles) n_tiles = tile_count(P.u.resolution[0], P.u.resolution[1]);
    const int form = 2 * kernel.instance + (P.u.use_tf ? 1 : 0);
    switch (form) {
#define HK_FORM(SLOT) \
    case 2 * SLOT: return render_tiles<FormCfg<SLOT, false>::type>(P, form, fb, tiles, n_tiles, first_sample, n_samples, kernel.samples_per_unit); \
    case 2 * SLOT + 1: return render_tiles<FormCfg<SLOT, true>::type>(P, form, fb, tiles, n_tiles, first_sample, n_samples, kernel.samples_per_unit);
    HK_FORM(0) HK_FORM(1) HK_FORM(2) HK_FORM(3) HK_FORM(4) HK_FORM(5) HK_FORM(6)
#undef HK_FORM
    default: return -1;
    }
}

#if defined(VR_HOST_TRACE)
// ---- L2 model (tests/tools_l2_breakdown.py, round 6): which class of access leaves one XCD's L2? ------------------------------------------------------------------
// A population of `population` paths -- what one XCD keeps in flight: 1024 wavefronts x 188 pool slots -- works through the pixel-samples of a band of the frame (an
// XCD's segment of the work queue is a contiguous band of tiles), every live path advancing by one state transition per round (a march pass of two DDA steps, a
// tentative collision, an event), so that the paths' accesses interleave as a population's do.  Every access the DEVICE makes in that transition is presented, with
// its device-layout address, to a model of the XCD's L2: `l2_bytes` in 128-byte lines, `ways`-way set associative, LRU, write-allocate without fetch.  The read-only
// tables report through the hooks in vr_trace.h (VR_TRACE); the cold path state (64-byte slots, the accesses the device scheduler makes: vr_pathtrace.h) and the
// sample pool are generated here.  Per class: accesses, accesses to a line other than the path's previous one of that class (what an L1 cannot merge), L2 misses.
// Not modelled: the L1s, the Infinity Cache, the scheduler's batching (a path waits for its event batch on the device).
}  // extern "C" (reopened below)
namespace {
enum SimClass { SC_MAJ_FINE = 0, SC_MAJ_COARSE, SC_TAP_DENSITY, SC_TAP_EMISSION, SC_ENV_WARP, SC_ENV_TEXEL, SC_COLD_READ, SC_COLD_WRITE, SC_SAMPLE_WRITE, SC_COUNT };
struct L2Model {
    uint32_t sets = 0, ways = 0;
    std::vector<uint64_t> tag;      // [set][way], 0 = empty; line address + 1
    std::vector<uint32_t> age;
    std::vector<uint8_t> dirty;
    uint32_t clock = 0;
    unsigned long long writebacks = 0;
    void init(size_t bytes, uint32_t w) { ways = w; sets = (uint32_t)(bytes / 128u / w); tag.assign((size_t)sets * w, 0); age.assign((size_t)sets * w, 0); dirty.assign((size_t)sets * w, 0); }
    // returns true on a hit
    bool access(uint64_t line, bool write) {
        const uint64_t h = line ^ (line >> 11) ^ (line >> 23);
        const size_t base = (size_t)(h % sets) * ways;
        ++clock;
        size_t victim = base; uint32_t oldest = 0xFFFFFFFFu;
        for (size_t i = base; i < base + ways; ++i) {
            if (tag[i] == line + 1) { age[i] = clock; if (write) dirty[i] = 1; return true; }
            if (tag[i] == 0) { victim = i; oldest = 0; }
            else if (oldest != 0 && age[i] < oldest) { victim = i; oldest = age[i]; }
        }
        if (tag[victim] != 0 && dirty[victim]) ++writebacks;
        tag[victim] = line + 1; age[victim] = clock; dirty[victim] = write ? 1 : 0;
        return false;
    }
};
struct SimSink {
    L2Model l2;
    unsigned long long acc[SC_COUNT] = {}, newline[SC_COUNT] = {}, miss[SC_COUNT] = {};
    uint64_t* last = nullptr;        // the current path's last line per class
    const void* density_table = nullptr; const void* emission_table = nullptr; const void* maj_table = nullptr;
    uint32_t maj_coarse_from = 0;    // first cell of majorant level 2
    bool paired = false;             // density and emission taps read ONE paired atlas (vr_scene.h pair_voxel_line)
    void touch(int cls, uint64_t space, uint64_t byte, uint32_t bytes, bool write) {
        const uint64_t l0 = byte >> 7, l1 = (byte + bytes - 1) >> 7;
        for (uint64_t l = l0; l <= l1; ++l) {
            const uint64_t line = (space << 40) | l;
            ++acc[cls];
            if (last && last[cls] == line + 1) continue;          // the line this path touched last in this class, in this transition: one instruction (or the L1) serves it
            if (last) last[cls] = line + 1;
            ++newline[cls];
            if (!l2.access(line, write)) ++miss[cls];
        }
    }
};
SimSink* g_sink = nullptr;
}  // namespace
namespace vr {
void host_trace(int32_t cls, const void* table, size_t a, size_t b) {
    SimSink* S = g_sink;
    if (!S) return;
    if (cls == TR_MAJORANT) {
        if (table != S->maj_table) return;                          // (the emission grid's majorant table is never read)
        S->touch(a >= S->maj_coarse_from ? SC_MAJ_COARSE : SC_MAJ_FINE, 1, (uint64_t)a * b, (uint32_t)b, false);
    } else if (cls == TR_TAP) {
        const bool em = table == S->emission_table;
        if (!em && table != S->density_table) return;
        // device layout: the paired atlas (ten 128-byte lines per brick: header + 56 (density, emission) voxel pairs each) or the grid's own brick-linear atlas
        // (five lines per brick: header + 120 voxels each); header and voxel come from ONE line
        const uint64_t line = S->paired ? (uint64_t)a * (kPairBlockBytes / 128u) + pair_voxel_line((uint32_t)b) : (uint64_t)a * (kBrickBlockBytes / 128u) + brick_voxel_line((uint32_t)b);
        S->touch(em ? SC_TAP_EMISSION : SC_TAP_DENSITY, (S->paired || !em) ? 2 : 3, line << 7, 4, false);
    } else if (cls == TR_ENV_WARP) {
        S->touch(SC_ENV_WARP, 4, a, (uint32_t)b, false);
    } else if (cls == TR_ENV_TEXEL) {
        S->touch(SC_ENV_TEXEL, 5, a, (uint32_t)b, false);
    }
}
}  // namespace vr
extern "C" {
// out: SC_COUNT x 3 counters (accesses, new-line accesses, L2 misses), then [27] dirty lines written back, [28] samples finished, [29] lane steps
long long hk_l2_breakdown(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                          const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim,
                          int x0, int y0, int x1, int y1, int spp, int population, long long l2_bytes, int ways, int paired, int lazy_emission,
                          unsigned long long* out, int n_bands) {
    // n_bands > 1: that many bands of y1 - y0 rows one after the other from y0 on (the frame's XCD segments), each with an L2 and a population of its own;
    // out then holds the bands' counters one after the other (32 words each)
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    const Uniforms& u = P.u;
    const int band_rows = y1 - y0;
    long long total = 0;
    for (int band = 0; band < (n_bands > 0 ? n_bands : 1); ++band, y0 += band_rows, y1 += band_rows, out += 32) {
    SimSink sink;
    sink.l2.init((size_t)l2_bytes, (uint32_t)ways);
    sink.density_table = P.density.atlas; sink.emission_table = u.has_emission ? P.emission.atlas : nullptr; sink.maj_table = P.density.majorant16;
    sink.maj_coarse_from = majorant_level_offset((uint32_t)(P.density.mshift[0] + P.density.mshift[1] + P.density.mshift[2]), 2u);
    sink.paired = paired != 0;
    struct Path { Hot h; ColdHost c; FirstStash stash; uint64_t last[SC_COUNT]; bool scattered; };
    std::vector<Path> paths((size_t)population);
    for (Path& p : paths) { hot_init(p.h); p.h.state = ST_NEW; memset(p.last, 0, sizeof p.last); p.scattered = false; memset(&p.c, 0, sizeof p.c); p.stash = FirstStash{}; }
    // work units: the 8x8 tiles of the band in raster order, all `spp` samples of a tile in one unit (the device's queue keeps a sub-tile's sample chunks adjacent)
    const int tx0 = x0 & ~7, ty0 = y0 & ~7;
    const int ntx = (x1 - tx0 + 7) / 8, nty = (y1 - ty0 + 7) / 8;
    const size_t n_units = (size_t)ntx * nty;
    std::vector<float> sbuf((size_t)64 * spp * 4, 0.0f);                       // (one unit's worth: the radiances themselves are not needed)
    size_t unit = 0;
    WorkUnit wu; uint32_t next_item = 0;
    auto open_unit = [&](size_t k) { wu.px0 = tx0 + 8 * (int)(k % ntx); wu.py0 = ty0 + 8 * (int)(k / ntx); wu.first_sample = 1; wu.n_items = 64 * spp; wu.base = 0u; wu.out = sbuf.data(); next_item = 0; };
    open_unit(0);
    const bool emission_on = u.has_emission != 0;
    unsigned long long finished = 0, steps = 0;
    g_sink = &sink;
    bool any = true;
    while (any) {
        any = false;
        for (size_t i = 0; i < paths.size(); ++i) {
            Path& p = paths[i];
            Hot& l = p.h;
            if (l.state == ST_DONE) continue;
            if (l.state == ST_NEW) {
                while (next_item >= (uint32_t)wu.n_items && unit + 1 < n_units) open_unit(++unit);
                if (next_item >= (uint32_t)wu.n_items) { l.state = ST_DONE; continue; }
                p.scattered = false;
                memset(p.last, 0, sizeof p.last);
            }
            any = true;
            memset(p.last, 0, sizeof p.last);                                  // merging only inside ONE transition (the dwordx4 loads of one block, a tap's header and voxel)
            sink.last = p.last;
            const uint64_t cold_byte = (uint64_t)i * 64u;                    // this slot's 64-byte cold slot in the XCD's share of the workspace
            const int32_t st = l.state;
            // the cold state as the DEVICE scheduler touches it (vr_pathtrace.h): a path has no cold line before its first scatter event (FirstStash; with an emission
            // grid: lazy_emission kernels); the collision event reads the line (not on a path's first) and writes sector 0, the scatter event reads it and writes
            // both sectors, the escape of a path that scattered reads it; emission kernels also read throughput and radiance when such a path is resumed for a
            // camera / scatter segment and write the radiance back when it is parked
            if (st == ST_NEE) { if (p.scattered) sink.touch(SC_COLD_READ, 6, cold_byte, 64, false); sink.touch(SC_COLD_WRITE, 6, cold_byte, p.scattered ? 32 : 64, true); }
            else if (st == ST_POSTNEE) { sink.touch(SC_COLD_READ, 6, cold_byte, 64, false); sink.touch(SC_COLD_WRITE, 6, cold_byte, 64, true); }
            else if (st == ST_ESCAPE) { if (p.scattered) sink.touch(SC_COLD_READ, 6, cold_byte, 64, false); sink.touch(SC_SAMPLE_WRITE, 7, finished * 16u, 16, true); }
            const int32_t shadow_before = l.shadow;
            if (u.use_tf) lane_step<TraceCfg<true, 2, 2, 2, 2>>(l, p.c, P, wu, next_item, p.stash); else lane_step<TraceCfg<false, 2, 2, 2, 2>>(l, p.c, P, wu, next_item, p.stash);
            ++steps;
            if (st == ST_NEE) p.scattered = true;
            if (emission_on && (lazy_emission ? p.scattered : true)) {
                // a camera / scatter segment begins (the path will be resumed: read thr + L) or ends (parked: write L) -- once per segment each
                if ((st == ST_POSTNEE || (st == ST_NEW && !lazy_emission)) && (l.state == ST_MARCH || l.state == ST_COLLIDE) && !l.shadow) sink.touch(SC_COLD_READ, 6, cold_byte, 32, false);
                if ((st == ST_MARCH || st == ST_COLLIDE) && !shadow_before && l.state != ST_MARCH && l.state != ST_COLLIDE) sink.touch(SC_COLD_WRITE, 6, cold_byte + 32u, 16, true);
            }
            if (st == ST_POSTNEE && l.state == ST_NEW) sink.touch(SC_SAMPLE_WRITE, 7, finished * 16u, 16, true);      // bounce cap / roulette: the scatter event writes the sample
            if (st == ST_ESCAPE || (st == ST_POSTNEE && l.state == ST_NEW)) { ++finished; }
            if (l.state == ST_NEW && st != ST_NEW) { /* the slot is free: it takes the next item in its next round */ }
        }
    }
    g_sink = nullptr;
    for (int c = 0; c < SC_COUNT; ++c) { out[3 * c] = sink.acc[c]; out[3 * c + 1] = sink.newline[c]; out[3 * c + 2] = sink.miss[c]; }
    out[27] = sink.l2.writebacks; out[28] = finished; out[29] = steps;
    total += (long long)finished;
    }
    return total;
}
#endif

void hk_set_trace(uint32_t* buf, unsigned long long cap) { g_trace = buf; g_trace_cap = (size_t)cap; g_trace_n = 0; }
unsigned long long hk_trace_count() { return (unsigned long long)g_trace_n; }

float hk_math(int fn, float x, float y) {
    switch (fn) {
    case 0: return log_(x); case 1: return sin_(x); case 2: return cos_(x); case 3: return tan_(x);
    case 4: return acos_(x); case 5: return atan2_(x, y); case 6: return exp_(x); case 7: return pow_(x, y);
    case 8: return asin_(x);
    case 13: { float s, c; sincos_(x, s, c); return s * y + c; }
    default: return nan_();
    }
}
}
