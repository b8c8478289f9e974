// vr_device.h -- the host-callable launchers of every HIP kernel (all asynchronous on `stream`), in sections, one per source file:
// vr_launch.hip (path tracing, features), vr_filters.hip (image space), vr_setup.hip (scene and environment), vr_probe.hip / vr_fastprobe.hip (test hooks).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_denoise.h"
#include "vr_scene.h"
#include "vr_temporal.h"
#include "vr_tiles.h"
#include "vr_variant.h"

namespace vr {

// ---- vr_launch.hip ---------------------------------------------------------------------------------------------------------------------------
// Path tracing: runs samples first_sample .. first_sample+n_samples-1 (1-based, the reference's current_sample)
// for every pixel of the listed 16x16 tiles (kernel 1: per-sample radiances into `sample_pool`) and folds them in
// sample order into the RGBA32F running mean `fb` (kernel 2; W*H texels, row 0 at the bottom).
// tiles == nullptr: all tiles of the frame (n_tiles = their count).  sample_pool must hold
// pathtrace_pool_floats(n_tiles, n_samples) floats; unit_counter is 8 device words (the work queue heads, one per XCD segment).  status[0] is set non-zero if a wavefront trips the watchdog.
// Tuning state of ONE renderer (nothing about a launch is process-global: two renderers, on one device or two, never share it).
struct PathtraceTuning {
    // scheduler thresholds, indexed like LaneState (vr_trace.h): NEW (free slots that trigger a NEW batch), [1] diagnostic cap on the slots in use
    // (0 = all), MARCH (= low-water mark of live paths: below it every non-empty batch runs), COLLIDE (lanes that must stand at a tentative
    // collision before the collision code runs while others still march; 0 = per kernel), NEE, POSTNEE, ESCAPE (batch sizes that trigger the event)
    int32_t thr[8] = { 64, 0, 56, 0, 60, 60, 64, 0 };
    unsigned long long* stats = nullptr;      // device buffer of 32 counters: the launch uses the instrumented (STATS) kernels; or null
    int32_t samples_per_unit = 0;             // samples of a work unit; 0 = per kernel variant
    int32_t blocks_per_cu = 0;                // resident workgroups per CU; 0 = from the occupancy query (cached per device)
    int32_t wide_addressing = 0;              // diagnostic (vr_set_int "wide_addressing"): 1 = the kernels with 64-bit gather addresses whatever the tables' sizes (vr_variant.h)
    bool operator==(const PathtraceTuning& o) const {
        for (int i = 0; i < 8; ++i) if (thr[i] != o.thr[i]) return false;
        return stats == o.stats && samples_per_unit == o.samples_per_unit && blocks_per_cu == o.blocks_per_cu && wide_addressing == o.wide_addressing;
    }
};
PathtraceTuning default_tuning();             // the defaults, with the diagnostic overrides VR_SPU / VR_BLOCKS_PER_CU of the environment (read once)
size_t pathtrace_pool_floats(const PathtraceTuning& T, int32_t n_tiles, int32_t n_samples);
size_t pathtrace_workspace_floats();      // cold path state of all resident wavefronts
void launch_pathtrace(const PathtraceTuning& T, const SceneParams& P, float* fb, float* sample_pool, float* workspace, uint32_t* unit_counter, const int32_t* tiles, int32_t n_tiles,
                      int32_t first_sample, int32_t n_samples, uint32_t* status, hipStream_t stream, bool fast_math = false,
                      hipEvent_t ev_kernel_begin = nullptr, hipEvent_t ev_kernel_end = nullptr,      // optional: bracket the path-tracing kernel alone
                      float* moments = nullptr,       // optional: W*H*4 per-channel second moments S = M2 / n, folded in the same pass (vr_set_int "variance")
                      // optional: the path seeds of samples 1..seed_samples of every pixel of the WHOLE frame (launch_seed_fill); the path-tracing kernel reads a
                      // new path's seed there instead of hashing it, and hashes for the samples beyond.  The other integrators hash always.
                      const uint32_t* seed_table = nullptr, int32_t seed_samples = 0,
                      // optional: the launch's CLEAR tiles (vr_sky_tiles.h; a device list, disjoint from `tiles`), whose samples of the same window sky_kernel
                      // renders into fb (and moments) without scheduler or pool, after the path-tracing kernel on the same stream and inside the same pair of
                      // events; it reads the same seed table.  n_tiles may be 0 then: no path-tracing kernel is launched and sample_pool, workspace and
                      // unit_counter are not touched.  A camera ray of theirs that hits the box sets kSkyHitStatus in status[0].
                      // n_see_tiles: the launch's SEE-THROUGH tiles, which follow the clear ones in sky_tiles and are rendered by the same launch without the box test
                      const int32_t* sky_tiles = nullptr, int32_t n_sky_tiles = 0, int32_t n_see_tiles = 0);
constexpr uint32_t kSkyHitStatus = 8u;
// Denoiser features of samples 1..spp for every pixel of the listed tiles (tiles == nullptr: all n_tiles of the frame): out = W*H*8 floats,
// (albedo.rgb, coverage, normal.xyz, depth) per pixel, row 0 at the bottom (vr_trace.h feature_pixel).  Pixels of other tiles are not written.
// status: the renderer's status word; a pixel whose tracker exceeded its step budget sets kFeatureLostStatus there (its remaining samples are not run).
constexpr uint32_t kFeatureLostStatus = 4u;
void launch_features(const SceneParams& P, const int32_t* tiles, int32_t n_tiles, int32_t spp, float* out, uint32_t* status, hipStream_t stream);
// The same buffer, same tiles, filled with the expected values of those features instead: rays x rays deterministic ray marches per pixel (vr_expected.h
// expected_pixel), rays in 1..kExpectedMaxRays.  Bounded by construction: no status word.
// clear: the clear-distance table of P.density (launch_clear_table), by which the march drops the steps of empty space -- same bits; nullptr, or a table without
// bytes: every step runs.  stats: 4 device counters that the launch ADDS to, in the instrumented twin of the kernel (sub-rays marched, steps reached, steps
// that fetched their corners, reads of the table); nullptr: the plain kernel.  cubic: march the tracker's field -- without a LUT the cubic B-spline field of
// vr_cubic.h, and clear must then be the table of reach 2; with a LUT the trilinear field, the same launch as without the flag.
constexpr int32_t kExpectedMaxRays = 4;
void launch_features_expected(const SceneParams& P, const int32_t* tiles, int32_t n_tiles, int32_t rays, float* out, hipStream_t stream,
                              const ClearTable* clear = nullptr, unsigned long long* stats = nullptr, bool cubic = false);
// which compiled kernel instance serves a scene, why, and whether it reads a seed table: vr_variant.h pathtrace_kernel_of
// fast_math: the opt-in tolerance-mode kernels (hardware transcendentals, reciprocal division; vr_math.h VR_FAST_MATH); the default
// kernels are bit-identical to the CPU oracle
// ---- vr_filters.hip --------------------------------------------------------------------------------------------------------------------------
// Denoiser (vr_denoise.h), whole W x H frames.  prepare: moments = W*H*4 Welford second moments S of n samples (the variance is S * vscale, 0 for
// n = 1: vr_variance's arithmetic), features = W*H*8 (vr_render_features) -> v = W*H variances of the mean's luminance, guide = W*H*8.
// atrous: one iteration of step `step` from (cin W*H*4, vin W*H, guide) into cout (W*H*4) and vout (W*H; nullptr: not written); the
// inputs and outputs must not overlap.
// counts: one sample count per raster tile (a frame of adaptive sampling), which replaces n and vscale per pixel; nullptr = the scalars.
// demod, here and on the split, the merge and the upsampling below ("denoise_demodulate" = 1, vr_demod.h): the kernel's DEMOD instance, which divides the layer and
// its standard deviation by the albedo of the same features, or multiplies it back; the arguments are the same.
void launch_denoise_prepare(const float* moments, const float* features, int32_t W, int32_t H, int32_t n, float vscale, const int32_t* counts, float* v, float* guide,
                            hipStream_t stream, bool demod = false);
void launch_denoise_atrous(const float* cin, const float* vin, const float* guide, int32_t W, int32_t H, int32_t step, const DenoiseSigma& sg,
                           float* cout, float* vout, hipStream_t stream);
// Temporal accumulation (vr_temporal.h), between prepare and the iterations, described by one struct.  The plain pass blends (color W*H*4, v W*H, guide
// W*H*8) with the history (hist_color W*H*4, hist_record W*H*4 = (V, N, K, D)) seen from camera `prev`, writes the new history into out_color / out_record
// (not the buffers read) and the integrated variance over v.  What else the struct carries picks the kernels:
//   out_moments set ("denoise_moments" = 1, vr_moments.h), two kernels: pass 1 also gathers and blends the moment records (hist_moments / out_moments, W*H*4 =
//     (m1, m2, E, S)), pass 2 forms S and V = S * E with the guide weights of `sigma` and writes V into out_record and over v.  The frame's own v is not read.
//   tau > 0 (the rejection test of vr_temporal.h steps 2a, 3a), two kernels with `scratch` between them, W*H*8 floats that nothing else here overlaps: W*H*4
//     of h, then W*H*4 of (v_h, N_h, z2, has).  Afterwards the first word of each of the latter holds the pixel's statistic T, -1 where it had no history.
// The launcher throws for a struct that asks for both, that asks for rejection without a scratch, or whose history pointers are not all set or all null.
struct TemporalPass {
    const float* color = nullptr;
    float* v = nullptr;
    const float* guide = nullptr;
    const float *hist_color = nullptr, *hist_record = nullptr, *hist_moments = nullptr;      // the previous history: all nullptr = none yet (hist_moments: with out_moments only)
    bool same_cam = false;                    // `cur` equals `prev` byte for byte (no reprojection)
    TemporalCamera cur{}, prev{};
    int32_t W = 0, H = 0;
    float alpha = 1.0f;
    float tau = 0.0f;                         // 0 = no rejection
    float* scratch = nullptr;                 // rejection only
    DenoiseSigma sigma{};                     // moments only
    float *out_color = nullptr, *out_record = nullptr, *out_moments = nullptr;
};
void launch_denoise_temporal(const TemporalPass& t, hipStream_t stream);
// The control variate of vr_resolve.h on the whole frame of P.u.resolution: fb (W*H*4, alpha = the share of samples that hit) and the coverage word of features
// (W*H*8, an expected-value pass of `rays` rays per axis) -> B (W*H*4: the environment behind each pixel, 0 with it hidden), Pq (W*H*4: the scattered part and its
// weight) and out (W*H*4: the resolved frame, alpha = the expected coverage).  Two kernels; no two arguments may overlap.
void launch_resolve(const SceneParams& P, const float* fb, const float* features, int32_t rays, float* B, float* Pq, float* out, hipStream_t stream);
// The layered filter of vr_layers.h on whole W x H frames.  split: y (W*H*4, the resolved frame), B (W*H*4, launch_resolve's) and the coverage word of features
// (W*H*8) -> S (W*H*4: the scattered layer, alpha = the coverage), which the denoiser's kernels read in the frame's place.  merge: F (W*H*4, their output), B and
// features -> out (W*H*4: the frame with the background back) and L (W*H*4: the layer).  One kernel each; outputs must not overlap inputs.
void launch_layers_split(const float* y, const float* B, const float* features, int32_t W, int32_t H, float* S, hipStream_t stream, bool demod = false);
void launch_layers_merge(const float* F, const float* B, const float* features, int32_t W, int32_t H, float* out, float* L, hipStream_t stream, bool demod = false);
// The one-pass regression of vr_regress.h on a whole W x H frame, in the place of the a-trous iterations: S (W*H*4: what iteration 0 would read, alpha = the
// coverage) and guide (W*H*8: launch_denoise_prepare's) -> F (W*H*4, what launch_layers_merge reads).  One kernel; F must not overlap the inputs.
void launch_denoise_regress(const float* S, const float* guide, int32_t W, int32_t H, const DenoiseSigma& sg, float ridge, float* F, hipStream_t stream);
// The upsampling of vr_upsample.h.  P: the scene with the HI resolution W x H = f w x f h (f in 2..4, or it throws); lo_layer (w*h*4: launch_layers_merge's L),
// lo_guide (w*h*8: launch_denoise_prepare's guide), hi_features (W*H*8: an expected-value pass at the hi resolution, `rays` rays per axis) -> out (W*H*4: the hi
// frame) and L (W*H*4: the hi layer).  One kernel; outputs must not overlap inputs.
void launch_upsample(const SceneParams& P, const float* lo_layer, const float* lo_guide, int32_t w, int32_t h, int32_t f, const float* hi_features, int32_t rays,
                     const DenoiseSigma& sg, float* out, float* L, hipStream_t stream, bool demod = false);
// Adaptive sampling (vr_adaptive.h): out[k] = e_t of raster tile tiles[k] holding counts[k] samples, k < n_tiles, from the W*H*4 framebuffer
// and the W*H*4 moments (device arrays, ids in range).
void launch_adaptive_error(const float* fb, const float* moments, const int32_t* tiles, const int32_t* counts, int32_t n_tiles, int32_t W, int32_t H, float* out,
                           hipStream_t stream);

// tonemap.glsl:29-36 in place
void launch_tonemap(float* fb, int32_t w, int32_t h, float exposure, float gamma, hipStream_t stream);

// multi-GPU shard helpers: copy owned 16x16 tiles frame <-> compact tile-major buffer (256 texels per tile)
void launch_pack_tiles(const float* fb, int32_t w, int32_t h, const int32_t* tiles, int32_t n_tiles, float* packed, hipStream_t stream);
void launch_unpack_tiles(const float* packed, const int32_t* tiles, int32_t n_tiles, float* fb, int32_t w, int32_t h, hipStream_t stream);
// the same for the denoiser's guides: moments (W*H*4) and features (W*H*8) <-> kGuidePlanes * 256 float4 per tile slot (vr_tiles.h guide_slot: wire format).
// pack: every tiles[k] a tile of the frame; unpack: tiles[k] < 0 = padding, the slot is not read
void launch_pack_guides(const float* moments, const float* features, int32_t w, int32_t h, const int32_t* tiles, int32_t n_tiles, float* packed, hipStream_t stream);
void launch_unpack_guides(const float* packed, const int32_t* tiles, int32_t n_tiles, float* moments, float* features, int32_t w, int32_t h, hipStream_t stream);
// ---- vr_setup.hip ----------------------------------------------------------------------------------------------------------------------------
// env_setup.glsl:18-34 + glGenerateMipmap (environment.cpp:27-31): importance pyramid of a dim x dim map
void launch_build_impmap(const float* envmap_rgba, int32_t env_w, int32_t env_h, int32_t dim, float* pyramid, hipStream_t stream);

// warp table of sample_environment: float4 per 2x2 block of every pyramid level (coarsest first); (dim^2 - 1) / 3 records
void launch_build_env_cdf(const float* pyramid, int32_t dim, float* table, uint32_t* unsafe_flag, hipStream_t stream);

// effective majorant of every cell of every range mip:
//   m = density_scale * float(range.y);  with a LUT: m = vol_majorant * tf_lookup(m * vol_inv_majorant).a
// (common.glsl:278-281, 425, 472)
void launch_majorants(const SceneParams& P, const uint32_t* range_words_all_mips, const int32_t nb[3], const int32_t mip_off[4], int32_t n_mips,
                      const int32_t mshift[3], float* out_padded, uint16_t* out16_padded, hipStream_t stream);      // out16: the raw fp16 range maxima, same layout

// Dense -> brick encoder on the device (Volume::to_brick_grid / commit(), src/renderer.cpp:63); see vr_setup.hip.
// ranges: range[nb] (fp16x2 words), flag[nb] (range is not a single value: the voxels matter)
void launch_encode_ranges(const float* dense, const int32_t dim[3], const int32_t nb[3], uint32_t* range, uint32_t* flag, hipStream_t stream);
void launch_encode_bricks(const float* dense, const int32_t dim[3], const int32_t nb[3], const uint32_t* range, const uint32_t* flag,
                          BrickRec* recs, float* rng, uint8_t* atlas, hipStream_t stream);      // rng: compact (rmin, rdiff) pairs, same index as recs
void launch_range_mip(const uint32_t* src, const int32_t sdim[3], uint32_t* dst, const int32_t ddim[3], hipStream_t stream);

// paired atlas of a density and an emission brick grid with the same brick layout (vr_scene.h kPairBlockBytes per brick); needs VR_BRICK_HEADERS blocks as input
void launch_pair_atlas(const uint8_t* atlas_density, const uint8_t* atlas_emission, uint8_t* out, size_t n_records, hipStream_t stream);

// decoded float atlas (one float per atlas byte: rmin + unorm8(b) * rdiff of its brick), used by transfer-function renders
void launch_decode_atlas(const float* rng, const uint8_t* atlas, float* out, size_t n_records, hipStream_t stream);
// Clear-distance table of the grid behind view g (vr_clear.h): table and scratch hold one byte per cell of clear_cells(g) each (vr_scene.h); the result is in table.
// reach: 1 (the trilinear lookup's table) or 2 (the cubic lookup's)
void launch_clear_table(const GridView& g, uint8_t* table, uint8_t* scratch, hipStream_t stream, int32_t reach = 1);
// Path-seed table (vr_tiles.h seed_table_index): the entries of the 0-based sample numbers [s_begin, s_end) of every pixel of the W x H frame's tiles, each
// vr_trace.h path_seed(seed, W, px, py, s + 1) -- what do_new hashes for that sample.  table holds s_end * tile_count(W, H) * 256 entries at least.
void launch_seed_fill(uint32_t* table, uint32_t seed, int32_t W, int32_t H, int32_t s_begin, int32_t s_end, hipStream_t stream);
// ---- vr_probe.hip, vr_fastprobe.hip ---------------------------------------------------------------------------------------------------------
// unit-test probe: out[i] = f(a[i], b[i]) with the device build of vr_math.h
// fn: 0 log 1 sin 2 cos 3 tan 4 acos 5 atan2 6 exp 7 pow 8 asin 9 a/b 10 sqrt 11 fma(a,b,a) 12 float(u8)/255 13 sincos 14 a*b+a 15 half->float
//     16 rcp_exact(a) 17 rcp3_exact((a, b, a)).y; 18.. : vr_math_probe.h
void launch_math_probe(int32_t fn, const float* a, const float* b, float* out, int32_t n, hipStream_t stream);
// the same over bit patterns: out[i] = f(bits(first + i), b), one launch, n <= 2^26 (fn 17 has no sweep form)
void launch_math_sweep(int32_t fn, uint32_t first, float b, float* out, int32_t n, hipStream_t stream);
// the VR_FAST_MATH forms (vr_fastprobe.hip, built with the tolerance-mode flags): 0 neg_log_1m(k 2^-24) 1 sincos_(bits(k)): s 2 the same: c 3 unorm8(k & 255), k = first + i
void launch_fast_math_sweep(int32_t fn, uint32_t first, float* out, int32_t n, hipStream_t stream);
// unit-test probe of the scene-data lookups (vr_probe.h, vr_probe.hip): n items of 4 words in, probe_out_words(what) floats out
void launch_probe(const SceneParams& P, int32_t what, int32_t form, const uint32_t* in, float* out, uint32_t n, hipStream_t stream);
// unit-test probe of the per-path layer (vr_path_probe.h, vr_probe.hip): n items of path_probe_in_words(kind) words in, path_probe_out_words(kind) words out
void launch_path_probe(const SceneParams& P, int32_t kind, int32_t form, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream);

}  // namespace vr
