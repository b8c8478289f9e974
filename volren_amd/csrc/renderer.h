// renderer.h -- RendererHIP: the MI355X drop-in for the reference's RendererOpenGL (src/renderer.h:16-63).
// Same public fields, same call protocol (mutate fields -> commit() after changing the volume -> reset() ->
// trace() once per sample, result = running mean in `color`, RGBA32F, row 0 at the bottom).  Differences that
// are visible to a caller are additions only:
//   * render(spp): all remaining samples in ONE fused launch (what bindings.cpp:124-132 loops over trace());
//   * trace() still advances `sample` by exactly one, but consecutive trace() calls on an unchanged scene are COALESCED
//     (round 5): the call records what it would launch -- a byte snapshot of every launch input -- and a following
//     trace() that finds the same bytes only adds to a count; the samples go out as ONE fused launch at the next
//     point where anyone could observe or change the frame (flush_pending()).  The reference's loop
//     `while (sample < sppx) trace();` (src/main.cpp:533-537, src/bindings.cpp:124-132) therefore runs at render(n)
//     speed, with the same bits,
//   * the camera and the resolution are explicit members instead of cppgl globals
//     (current_camera(), Context::resolution(): renderer.cpp:47,93-95,137),
//   * set_tiles(): restrict a renderer to a subset of 16x16 framebuffer tiles (multi-GPU sharding).
#pragma once

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "devmem.h"
#include "environment.h"
#include "grids.h"
#include "transferfunc.h"
#include "vr_device.h"
#include "vr_regress.h"
#include "vr_scene.h"

namespace vr {

struct SkyLiveCells;                       // vr_sky_tiles.h (host only)

// stand-in for cppgl's camera (pos/dir/up/fov_degree are what the renderer reads: renderer.cpp:93-95)
struct Camera {
    vec3 pos{ 1.f, 0.f, 1.f };                 // main.cpp:458
    vec3 dir = normalize(-pos);                // main.cpp:459 (note dir.y = -0.f, as in the reference)
    vec3 up{ 0.f, 1.f, 0.f };
    float fov_degree = 70.f;                   // cppgl default (unverified): always pass --cam_fov
    mat3 view_inverse() const;                 // inverse(mat3(lookAt(pos, pos+dir, up))): columns right, up, -forward
};

// replaces BrickGridGL (renderer.h:9-14): the three textures become three device arrays (+ majorant cache)
struct BrickGridHIP {
    DeviceBufferPtr bricks;        // BrickRec per brick
    DeviceBufferPtr atlas;         // brick-major u8 voxels, 512 B per slot
    DeviceBufferPtr range_words;   // fp16x2 range of every cell of mips 0..n_mips (input of the majorant kernel)
    DeviceBufferPtr majorant;      // effective majorants (float), padded power-of-two layout (vr_scene.h)
    DeviceBufferPtr majorant16;    // raw fp16 range maxima in the same layout (read by the kernels without a transfer function)
    DeviceBufferPtr rng;           // compact (rmin, rdiff) float pairs, same index as `bricks` (what a tap reads)
    DeviceBufferPtr atlas_f32;     // decoded float atlas, built on the first render with a transfer function (4x the atlas; dropped by commit())
    bool atlas_f32_failed = false; // its allocation failed once: not retried until commit() or a tf_float_atlas toggle (the byte atlas serves)
    DeviceBufferPtr atlas_paired;  // this grid's voxels interleaved with those of the frame's other grid (density + emission grids of one brick layout: vr_scene.h);
                                   // one buffer, held by both grids of the frame; built by commit()
    DeviceBufferPtr clear_table[2];// clear-distance tables (vr_clear.h) of reach 1 and 2, one byte per cell, each built by the first expected-value pass that
                                   // marches this grid with it; a grid that commit() uploads anew starts without them
    DeviceBufferPtr dense;         // dense fp16 voxels in 4x4x4 blocks (DenseGridF16), then bricks/atlas are empty
    int32_t dim[3] = { 0, 0, 0 };
    int32_t dblk[2] = { 0, 0 };            // 4x4x4 blocks per axis (x, y) of the dense layout
    int32_t nb[3] = { 0, 0, 0 };
    int32_t mip_off[4] = { 0, 0, 0, 0 };   // word offset of each level inside range_words (compact)
    int32_t n_mips = 0;
    int32_t n_cells = 0;                   // words in range_words
    int32_t mshift[3] = { 3, 3, 3 };       // padded power-of-two extent of `majorant` (vr_scene.h)
    size_t n_active = 0;                   // bricks whose voxels matter (range not a single value): what the choice of the majorant layout looks at
    bool maj_blocked = false;              // commit()'s choice for this grid: majorant levels 0-1 in 4x4x4-cell blocks (vr_scene.h majorant_cell_index)
    std::shared_ptr<const SkyLiveCells> live_cells;   // which cells of the host grid's range table can hold density > 0 (vr_sky_tiles.h), for the see-through tiles of a
                                           // density grid; null for a grid whose table the host does not hold (encoded on the device): no see-through tile then
    mat4 transform;
};

struct RendererHIP {
    // Renderer interface
    void init();
    void resize(uint32_t w, uint32_t h);
    void commit();
    void trace();
    void draw();
    void reset();

    // all of `n` further samples in one launch (n <= 0: up to sppx)
    void render(int n = 0);
    // Adaptive sampling (vr_adaptive.h): every tile of the tile set (set_tiles; empty = the whole frame) to min_spp, then rounds that evaluate
    // the error e_t of the tiles below max_spp, retire those with e_t < threshold and double the others' counts (at most max_spp).  Starts from
    // a uniform frame of `sample` samples (whose moments cover it, unless sample = 0) or from the counts a previous call left.  Keeps the moments
    // for all its launches whatever `variance` says (the field is left unchanged).  Afterwards sample = the largest count of any tile; a frame
    // whose tiles hold different counts is "ragged" (tile_samples) until sample changes.  Asynchronous like render(), except that every round
    // waits for its error values (one small copy) and throws on a tripped watchdog.  2 <= min_spp <= max_spp, threshold finite and >= 0.
    void render_adaptive(int min_spp, int max_spp, float threshold);
    // samples behind every raster tile (tiles_x * tiles_y, row 0 = bottom): `sample` everywhere on a uniform frame
    std::vector<int32_t> tile_samples();
    // e_t of every raster tile at its current count (the schedule's kernel); needs moments that cover the frame.  Waits
    std::vector<float> tile_error();
    bool ragged();                                     // the frame holds the per-tile counts of a render_adaptive (drops them once `sample` has moved)
    void drop_tile_samples();                          // forget them (vr_set_int "sample": a value set back by hand does not revive them)
    void check_watchdog();                             // throws (as vr_synchronize reports it) if the status word is set; reads and clears it

    // helper to convert brick grid to device arrays
    BrickGridHIP brick_grid_to_device(const std::shared_ptr<BrickGrid>& grid);
    BrickGridHIP dense_grid_to_device(const std::shared_ptr<DenseGridF16>& grid);
    BrickGridHIP grid_to_device(const Volume::GridPtr& grid);      // dense fp16 stays dense, everything else becomes bricks
    BrickGridHIP dense_to_bricks_on_device(const std::shared_ptr<DenseGrid>& grid);   // to_brick_grid + upload, all on the GPU
    bool gpu_encoder = true;                                       // DenseGrid -> bricks on the device (false: host encoder)
    void grid_checksums(const BrickGridHIP& g, uint64_t out[3]) const;   // FNV-1a of bricks / atlas / range words (tests)
    // scale and move volume to fit into [-0.5, 0.5] unit cube
    void scale_and_move_to_unit_cube();

    // General settings
    int sample = 0;
    int sppx = 1024;
    int seed = 42;
    int bounces = 100;
    float tonemap_exposure = 5.f;
    float tonemap_gamma = 2.2f;
    bool tonemapping = true;
    bool show_environment = true;

    // Volume settings
    vec3 albedo = vec3(0.9f);           // volume albedo
    float phase = 0.f;                  // volume phase (henyey-greenstein g parameter)
    float density_scale = 1.f;          // volume density scaling factor
    float emission_scale = 100.f;       // volume emission scaling factor

    // device data
    DeviceBufferPtr color;              // RGBA32F running mean, W*H texels, row 0 = bottom
    DeviceBufferPtr display;            // tonemapped copy written by draw()
    std::vector<BrickGridHIP> density_grids;
    std::vector<BrickGridHIP> emission_grids;
    float majorant_emission = 0.f;

    // Volume data
    std::shared_ptr<Volume> volume;

    // Volume clip planes
    vec3 vol_clip_min = vec3(0.f);
    vec3 vol_clip_max = vec3(1.f);

    // Scene data
    std::shared_ptr<Environment> environment;
    std::shared_ptr<TransferFunction> transferfunc;

    // ---- additions ----
    Camera camera;
    ivec2 resolution{ 0, 0 };
    hipStream_t stream = nullptr;
    int integrator = 0;                               // 0: DDA tracking (both reference kernels), 1: global-majorant tracking (common.glsl:333-394),
                                                      // 2: direct volume rendering (:571-591, needs a LUT), 3: 64-step ray-marching trackers (:506-566)
    bool tf_float_atlas = true;                       // transfer-function renders decode the brick atlas to floats once (4x its size): one load per corner tap
    int order_tiles = 1;                              // a launch works through its tiles costliest first (chord of the pixel rays through the volume's box), so that what
                                                      // is left when the work queue runs empty are short paths (profiles/r4f_*): 0 never, 1 when the renderer has a tile
                                                      // subset (a rank's share: +0.5 ... +7 %), 2 always (full frames measure +-0.5 %: raster order stays their default).
                                                      // Which tile runs when never changes a result
    int majorant_layout = -1;                         // layout of the majorant table's levels 0-1 for the frames the two-brick-grid kernel serves: -1 = per grid, chosen at
                                                      // commit() (blocked when more than kBlockedMajorantBricks bricks carry voxels: the large, well filled sparse grids of
                                                      // BASELINE configs[4], +3 % there, -2 % on small or thinly filled ones: profiles/r4d_*, r5_*), 0 = linear, 1 = blocked.
                                                      // Results never depend on it
    int variance = 0;                                 // 1: every accumulation pass also keeps the per-channel second moments of the samples (download_variance)
    int denoise_iterations = kDenoiseDefaultIterations;   // a-trous iterations of denoise() (0..kDenoiseMaxIterations; 0 = the colour unchanged)
    float denoise_sigma[5] = { kDenoiseDefaultSigma[0], kDenoiseDefaultSigma[1], kDenoiseDefaultSigma[2], kDenoiseDefaultSigma[3], kDenoiseDefaultSigma[4] };
                                                      // edge-stopping widths: colour, normal, depth, coverage, albedo (vr_denoise.h)
    float denoise_alpha = kTemporalDefaultAlpha;      // smallest weight of the current frame in denoise_temporal()'s blend, in [2^-20, 1] (vr_temporal.h)
    int denoise_moments = 0;                          // 1: denoise_temporal() takes the filter's variance from luminance moments kept in the history (vr_moments.h); set it with set_denoise_moments
    float denoise_reject = 0.0f;                      // threshold tau of denoise_temporal()'s history rejection (vr_temporal.h 2a, 3a): 0 = off, or in [2^-10, 2^20]
    bool fast_math = false;                           // opt-in tolerance mode: hardware log/sin/cos/rcp instead of the specified arithmetic
                                                      // (not bit-reproducible; without a transfer function within 1e-3 relative L2 of the default --
                                                      // with one bound the renderer refuses it: DESIGN.md 3)
    PathtraceTuning tuning = default_tuning();        // scheduler thresholds, work-unit size, statistics buffer of THIS renderer's launches
    int sky_tiles = 1;                                // 1: a submit's CLEAR tiles -- 16x16 tiles no camera ray of which can hit the volume's box (vr_sky_tiles.h), whose samples
                                                      // are all (environment, alpha 0) -- are rendered by one thread per pixel (vr_launch.hip sky_kernel) instead of going through the
                                                      // path scheduler and the sample pool; the path tracer gets the other tiles.  The split depends on camera, box and frame size alone;
                                                      // a view without clear tiles is launched as with 0.  Off, whatever this says, while the instrumented kernels are on (sched_stats:
                                                      // every sample passes through them), in the tolerance mode (fast_math: its frames belong to that build's arithmetic) and for the
                                                      // item integrators (2, 3).  Results never depend on it
    int last_sky_tiles = 0;                           // clear tiles of the last submit (0: it was not split)
    int see_through_tiles = 1;                        // 1: where the clear tiles are split off (sky_tiles says where), so are a submit's SEE-THROUGH tiles -- tiles whose rays surely cross the
                                                      // box but cannot come within tap reach of a cell of the density grid that holds density > 0 (vr_sky_tiles.h): every sample of
                                                      // theirs is (environment, alpha 0) as well, and the same kernel renders them without the box test.  Only for integrators 0 and 1
                                                      // without emission grid and transfer function, a finite density scale >= 0 and a grid whose range table the host holds; a view
                                                      // without such tiles is launched as with 0.  Results never depend on it
    int last_see_through_tiles = 0;                   // see-through tiles of the last submit (last_sky_tiles counts the clear ones only)
    int last_launches = 0;                            // path-tracing sub-launches of the last trace()/render()/render_adaptive()
    int adaptive_rounds = 0;                          // error evaluations (rounds) of the last render_adaptive()
    int launch_target_ms = 2000;                      // a sub-launch is planned to take at most this long, from the rate the renderer measured on its last launch (a short
                                                      // probe launch when it has none for the current settings and the request is large); 0 = plan by the sample pool alone.
                                                      // Correctness does not depend on it (the kernel's watchdog is progress-based): it bounds how long one launch holds the GPU
    size_t sample_pool_bytes = (size_t)64 << 30;      // HBM budget of the per-sample radiance pool (16 B per pixel-sample; sized for 288 GB HBM3E: 64 GiB = the 2^32 items a sub-launch
                                                      // can index; allocated on demand, only as large as a launch needs, halved when it does not fit the free memory).  Round 5: 16 -> 64 GiB,
                                                      // a 2048^2 x 4096-spp frame is 5 sub-launches instead of 16 and each one's drain (4-8 ms) is paid that much less often: c5full +2.2 %,
                                                      // c4 at 1920x1080x4096 +0.9 % (tests/tools_pool_ab.py)

    // Path-seed table.  A new path's RNG state is a 32-round hash of (seed, W, pixel, sample number) and of nothing else, and those stay the same from frame to
    // frame -- progressive refinement starts over at sample 1 after every camera move, a script renders frame after frame at one seed and size -- so the renderer
    // keeps the hashes of the whole frame's first samples in a device table (vr_tiles.h seed_table_index; 4 bytes per pixel of the tile grid and sample) and the
    // path-tracing kernel reads a seed where it would compute it.  The table is keyed by (seed, W, H): reset() keeps it, a change of any of the three drops it.  It
    // grows to the sample numbers launches have asked for, up to the budget; before a launch the part of its sample range that is not covered yet is filled on the
    // launch's stream.  Samples beyond the budget hash in the kernel, as do the feature passes, the other integrators and the kernels that measured no faster with
    // it (dense grids, emission grids, the run-time variant: vr_pathtrace.h seed_request_point) always -- their launches make no table; a table that cannot be
    // allocated is given up (said once) and the renderer hashes as before: no render fails for it.  Results do not depend on any of this.
    // seed_table_mb: the budget in MiB, 0 = no table, -1 = min(4096, sample_pool_mb / 4) -- a 1024^2 frame of 1024 spp is covered in full, and a renderer whose
    // pool was made small stays small.  The parts of a ShardedRenderer each hold a table of their own, indexed by the whole frame's tiles: n parts on one device
    // cover the frame's samples n times over within n budgets (left so: parts on a device of their own are the case the sharded renderer is for).
    int seed_table_mb = -1;
    int seed_table_max_samples = 0;                         // > 0: the table covers at most this many samples per pixel, whatever the budget allows (0: the budget alone decides)
    static constexpr int kSeedTableMaxMb = 8192;            // 2^31 entries: the kernels index the table in 32 bits
    static int seed_table_default_mb(long long sample_pool_mb) { return (int)std::min<long long>(4096, sample_pool_mb / 4); }
    static int seed_table_samples_for(long long mb, int w, int h);      // sample numbers a budget covers on a w x h frame
    int seed_table_budget_mb() const { return seed_table_mb >= 0 ? seed_table_mb : seed_table_default_mb((long long)(sample_pool_bytes >> 20)); }
    int seed_table_samples() const { return seed_filled_; }    // sample numbers 1..this of the current (seed, W, H) are in the table now
    int seed_table_fills() const { return seed_fills_; }       // fill launches so far (diagnostics, tests)
    void set_tiles(const std::vector<int32_t>& tile_ids);     // empty = whole frame
    void fill_params(SceneParams& P);                          // renderer.cpp:88-138
    void download(float* rgba);                                // color -> host
    // Denoiser data.  render_features(spp): the first-scatter features of samples 1..spp of every pixel of the tile set (vr_trace.h feature_pixel),
    // computed afresh into their own W*H*8 buffer (asynchronous; flushes recorded samples first).  download_features: that buffer, W*H*8 floats.
    // download_variance: the unbiased per-channel variance of samples 1..sample, W*H*4 floats -- needs `variance` on for all of them.
    // render_features_expected(rays): the expected values of the same features from rays x rays deterministic ray marches per pixel (vr_expected.h
    // expected_pixel; rays in 1..4) into the same buffer -- the limit of render_features for spp -> infinity, without noise, at a cost independent of spp.
    // Counts as a feature pass for everything that needs one.
    // expected_skip = 1: the march reads the density grid's clear-distance table (vr_clear.h) and drops the steps of empty space with their loads -- the
    // same bits as 0, which runs every step.  The table is built on the device when the first such pass reads a grid (each frame of an animation has its
    // own; commit() drops them all): renders that never ask for the pass pay nothing.  expected_stats = 1: the passes count their work in the
    // instrumented twin of the kernel; expected_stats_read waits and returns the last pass's totals (sub-rays marched, steps reached, steps that fetched
    // their corners, table reads), and throws when that pass did not count.  expected_clear_table: test hook, the current density grid's table (built if
    // need be) and its extent in cells; out may be null.
    // expected_field = 1: every expected-value pass (this one, a tile subset's, upsample()'s) marches the field the tracker decides its collisions on: without a
    // LUT the cubic B-spline field of vr_cubic.h (64 taps a step; the clear-distance table of reach 2), with a LUT the trilinear one -- the same bits as 0, the
    // default, which marches the trilinear field always.  Changing it drops no temporal history: the next pass is simply another guide.  expected_clear_table
    // returns the table the current setting marches with.
    void render_features(int spp);
    void render_features_expected(int rays);
    int expected_field = 0;
    int expected_skip = 1;
    int expected_stats = 0;
    void expected_stats_read(uint64_t out[4]);
    void expected_clear_table(uint8_t* out, int cells[3]);
    // test hook (vr_probe.h): n items of probe `what` in compile-time form `form`, host arrays in (4 words per item) and out (probe_out_words floats per item), run by
    // probe_kernel on the SceneParams the next launch would get -- after capture() (float atlas) and update_majorants, with the paired atlas where a kernel reads it.
    // Throws for a form the scene cannot serve.  Synchronous; touches no framebuffer.
    void probe(int what, int form, const uint32_t* in, float* out, size_t n);
    // test hook (vr_path_probe.h): the same for the per-path layer -- n items of path_probe_in_words(kind) words in, path_probe_out_words(kind) words out.  A segment
    // form is a compiled instance: the paired-atlas instances (4, 5) read the paired views, every other form the grids' own atlases.
    void path_probe(int kind, int form, const uint32_t* in, uint32_t* out, size_t n);
    // test hook (include/volren_amd.h vr_filter_probe: the stages, the arrays and the parameter block): one launch_* of vr_device.h's vr_filters.hip section on
    // host arrays, through fresh device buffers on this renderer's stream.  The arguments are checked by the caller (capi.cpp).  Synchronous; touches no buffer,
    // flag or history of the renderer.
    void filter_probe(int stage, int W, int H, const void* const* in, float* const* out, const float* params);
    void download_features(float* out);
    void download_variance(float* rgba);
    // Denoiser (vr_denoise.h).  denoise(): the a-trous filter of the current frame, guided by the variance and the last feature pass, into its own W*H*4
    // buffer (asynchronous; flushes recorded samples first).  Needs render_features since the last resize, `variance` on for samples 1..sample, sample >= 1
    // and no tile subset.  download_denoised: that buffer, W*H*4 floats.  The framebuffer, moments, features and display are not touched.
    // denoise_temporal() (vr_temporal.h): the same, with the frame first blended into a history of the frames before it, reprojected by the guide's
    // depth from the camera of the call before (once per frame; frames of equal spp).  Whatever denoise() accepts, this accepts.  The history is created
    // by the first call, dropped by resize and drop_history, and kept across everything else; denoise() neither reads nor writes it.
    // download_history: integrated colour W*H*4, integrated variance W*H, length W*H (any may be null); throws while there is no history.
    // With denoise_reject > 0 a pixel whose history disagrees with the frame beyond the noise of the two starts afresh (other kernels, one scratch buffer
    // more; 0 is today's call exactly).  download_reject_stat: W*H statistics T of the last denoise_temporal(), -1 where the pixel had no history; throws
    // unless the last denoise_temporal() since the resize ran with denoise_reject > 0.
    // With denoise_moments = 1 the history carries a third array, the moment record (m1, m2, E, S) of the frames' luminance, and the variance the
    // iterations start from is S * E instead of the blend of the frames' sample variances: frames of 1 spp, which have none, are filtered (other kernels;
    // 0 is today's call exactly).  set_denoise_moments: 0 or 1, throws otherwise; a change drops the history (one without moment records cannot continue
    // one with them).  Together with denoise_reject > 0 denoise_temporal() throws before anything is launched: the rejection statistic needs a sample
    // variance.  download_history_moments: W*H*4 floats; throws unless the current history was written with denoise_moments = 1.
    // Several devices: ShardedRenderer::denoise / denoise_temporal (sharded.h); called on a part directly, these refuse the part's tile subset.
    void denoise();
    void denoise_temporal();
    void drop_history();
    // The control variate on the expected coverage (vr_resolve.h).  resolve(): the frame with its hit/miss noise replaced by the feature buffer's expected
    // coverage, y = x + beta (alpha - kappa), into its own W*H*4 buffer (asynchronous; flushes recorded samples first).  Throws, before anything is launched,
    // when sample < 1, a tile subset is set, integrator = 2 (its alpha is an opacity, not a hit indicator), or the feature buffer was not last filled -- since
    // the last resize -- by render_features_expected with rays >= 2.  Ragged frames are fine: only means are used.  The framebuffer, features, moments and
    // display are not touched.  download_resolved: that buffer, W*H*4 floats, alpha = kappa.  download_resolve_background: B, the environment behind every pixel
    // as the last resolve() formed it (W*H*4, alpha 0; test hook).  Both throw before the first resolve since the last resize.
    // denoise_resolve = 1: denoise() and denoise_temporal() -- with rejection and with moments too -- run resolve() first and start from its result instead of
    // the framebuffer's colour, the frame's variance unchanged; whatever resolve() refuses they refuse then (0 is today's calls exactly).
    // set_denoise_resolve: 0 or 1, throws otherwise; a change drops the history.
    void resolve();
    void check_resolve(const std::string& me, bool whole_frame_gathered);      // resolve()'s refusals, from host state alone: throws, launches nothing
    void download_resolved(float* rgba);
    void download_resolve_background(float* rgba);
    void set_denoise_resolve(int v);
    int denoise_resolve = 0;
    // The layered filter (vr_layers.h).  denoise_layers = 1: denoise() and denoise_temporal() -- with rejection and with moments too -- run resolve()'s two kernels
    // (whatever denoise_resolve says), split the resolved frame into the background's share and the scattered layer, filter the layer with the frame's own variance,
    // and merge: the layer renormalised by the exact coverage, the analytic background added back.  The history then holds the layer, not the composite.  Whatever
    // resolve() refuses they refuse then, before anything is launched (0 is today's calls exactly: the same launches, allocations and results).
    // set_denoise_layers: 0 or 1, throws otherwise; a change drops the history.  download_denoised_layer: the layer of the last such call, W*H*4 floats: scattered
    // light premultiplied by the exact coverage, alpha = the coverage; throws before the first such call since the last resize.
    void set_denoise_layers(int v);
    int denoise_layers = 0;
    void download_denoised_layer(float* rgba);
    // The one-pass regression (vr_regress.h).  denoise_filter = 1: with denoise_layers = 1, one 11 x 11 pass of weighted local regression on the scattered layer
    // takes the place of the a-trous iterations of denoise() and denoise_temporal(); resolve, split, the temporal pass with rejection or moments and the merge stay
    // as they are, denoise_iterations = 0 still leaves the layer unfiltered, and the variance is neither read nor written by the pass.  Without denoise_layers = 1
    // the calls throw before anything is launched, and whatever denoise_layers refuses they refuse (0 is today's calls exactly).  set_denoise_filter: 0 or 1,
    // throws otherwise; a change drops the history.  denoise_ridge: the ridge lambda on the fit's seven slopes, 0 (zero order: the normalised weighted mean) or
    // in [2^-20, 2^20]; set_denoise_ridge throws for anything else.
    void set_denoise_filter(int v);
    int denoise_filter = 0;
    void set_denoise_ridge(float v);
    float denoise_ridge = kRegressDefaultRidge;
    // Albedo demodulation (vr_demod.h).  denoise_demodulate = 1: with denoise_layers = 1, the split divides the scattered layer by the albedo of the feature buffer
    // (floored at 2^-6, 1 where the coverage is 0), prepare divides the channels' standard deviations alike, the filter -- iterations or regression, the temporal
    // pass with rejection or moments -- runs on the quotient, the history holds it, and the merge multiplies back: the DEMOD instances of the same kernels, no
    // launch and no buffer more.  The layer keeps its meaning.  upsample() with the setting 1 at its call demodulates the lo layer by the lo guide inside its kernel
    // and remodulates by the hi guide, whatever produced the layer.  Without denoise_layers = 1 denoise() and denoise_temporal() throw before anything is launched
    // (0 is today's calls exactly).  set_denoise_demodulate: 0 or 1, throws otherwise; a change drops the history.
    void set_denoise_demodulate(int v);
    int denoise_demodulate = 0;
    // The layer upsampled under a full-resolution guide (vr_upsample.h).  upsample(factor, rays): the frame at factor x the renderer's size per axis, rebuilt from
    // the layer of the last denoise() / denoise_temporal() with denoise_layers = 1 and an expected-value pass of `rays` rays per axis at that size, which the call
    // marches into a buffer of its own with the scene and camera as they are now -- the caller keeps them as they were at the denoise call.  expected_skip and
    // expected_stats act on that pass as on render_features_expected.  Asynchronous; flushes recorded samples first.  factor in 2..4, rays in 1..4.  Throws, before
    // anything is launched, when download_denoised_layer would, or when a tile subset is set (unless the layer is a gathered whole frame's: part 0 of a
    // ShardedRenderer).  The first call allocates the hi buffers; resize drops them, and so does a call with another factor.  The framebuffer, the lo feature
    // buffer with what says which pass filled it, the filter's results and the history are not touched.
    // download_upsampled / download_upsampled_layer: the hi frame and the hi layer, W*H*4 floats each; download_upsampled_features: the hi feature buffer, W*H*8,
    // bit for bit render_features_expected's of a renderer resized to W x H.  upsampled_size: (W, H).  All four throw before the first upsample since the last resize.
    void upsample(int factor, int rays);
    void download_upsampled(float* rgba);
    void download_upsampled_layer(float* rgba);
    void download_upsampled_features(float* out);
    void upsampled_size(int wh[2]) const;
    const DeviceBuffer* upsampled() const { return sized_.up_factor ? sized_.up_out.get() : nullptr; }
    void download_history(float* rgba, float* var, float* length);
    void download_reject_stat(float* out);
    void set_denoise_moments(int v);
    void download_history_moments(float* out);
    void download_denoised(float* rgba);
    const DeviceBuffer* denoised() const { return sized_.denoised.get(); }
    const DeviceBuffer* resolved() const { return sized_.resolved.get(); }
    // copy + tonemap of a W*H*4 buffer into `display` (draw() = draw_from(*color) after the flush)
    void draw_from(const DeviceBuffer& src);
    void download_display(float* rgba) const;
    void synchronize();
    // Launches the samples that coalesced trace() calls have recorded (no-op without any).  Every member function that reads or replaces the
    // framebuffer, the device grids, the tile set or the timing state calls it first (render, draw, download, synchronize, commit, resize,
    // set_tiles, last_*_ms, sched_stats, watchdog_status, ...); a caller that reads `color` through its raw device pointer calls it itself
    // (the C ABI does: vr_framebuffer_device, vr_pack_tiles, vr_unpack_tiles, vr_set_stream).  Changes of PUBLIC FIELDS between two trace()
    // calls need no flush by the caller: the next trace() sees bytes that differ from the recorded ones and launches the recorded samples first,
    // with the values they were recorded with.
    void flush_pending();
    int begin_feature_pass(SceneParams& P);      // the common head of render_features / render_features_expected (renderer.cpp)
    void feature_scene(SceneParams& P);          // its first half, which upsample() shares: the scene as a feature pass reads it; touches no feature buffer
    // the expected-value pass both callers launch: the clear-distance table and the counters as expected_skip / expected_stats say, then the kernel over `tiles`
    void launch_expected(const SceneParams& P, const int32_t* tiles, int n_tiles, int rays, float* out);
    int pending_samples() const { return pending_n_; }         // samples recorded by trace() and not launched yet
    bool coalesce_trace = true;                                // false: every trace() is its own launch (round 4's behaviour; A/B and tests)
    double last_kernel_ms();                                    // HIP-event time of the last launch (a render(), or the trace() calls coalesced into one): all sub-launches, path tracing + accumulation (waits for it)
    double last_pathtrace_ms();                                 // HIP-event time of the path-tracing kernel alone, summed over the sub-launches of the last trace()/render()
                                                                // (0 when that call launched none: integrators 2 / 3)
    void sched_stats(bool enable, unsigned long long out[32]);
    void wave_timeline(unsigned long long* out, size_t n_words);  // diagnostics: the per-wavefront (begin, queue empty, end) triples of the last instrumented launch  // diagnostics: out (may be null) receives the counters gathered so far; enable starts (zeroed) or stops counting
    uint32_t watchdog_status();
    ~RendererHIP();

private:
    // majorant cache key
    struct MajKey {                                                // tf_version: TransferFunction::version (unique per upload), 0 = no LUT
        float density_scale = -1.f; uint64_t tf_version = ~0ull; float wl = 0, ww = 0; size_t frame = ~(size_t)0; int blocked = -1;
        // (field by field: the padding is not zeroed)
        bool operator==(const MajKey& o) const { return density_scale == o.density_scale && tf_version == o.tf_version && wl == o.wl && ww == o.ww && frame == o.frame && blocked == o.blocked; }
    };
    // Everything a launch reads from the renderer's mutable state, as one trace()/render() call found it.  `P` is zero-filled before it is written
    // (fill_params), so two snapshots are compared byte by byte; the handles keep alive what P points into (a caller may replace the environment or
    // re-upload the LUT between two trace() calls: the recorded samples still see the old arrays, as the reference's already issued dispatches do).
    struct LaunchInputs {
        SceneParams P;
        MajKey maj;
        size_t frame = 0;
        PathtraceTuning tuning;
        int order_tiles = 0, launch_target_ms = 0, fast_math = 0, variance = 0, sky_tiles = 0, see_through_tiles = 0;
        size_t sample_pool_bytes = 0;
        hipStream_t stream = nullptr;
        std::shared_ptr<Environment> env;
        std::shared_ptr<TransferFunction> tf;
        DeviceBufferPtr keep[5];               // envmap, impmap, env_cdf, lut, compact envmap
        bool same_launch_as(const LaunchInputs& o) const;
        PathtraceKernel kernel() const { return pathtrace_kernel_of(P, tuning.wide_addressing != 0, tuning.stats != nullptr); }      // the kernel that serves the launch (vr_variant.h)
        // the launch's clear tiles are split off (RendererHIP::sky_tiles says when not)
        bool splits_sky() const { return sky_tiles != 0 && tuning.stats == nullptr && fast_math == 0 && kernel().item_integrator == 0; }
    };
    void capture(LaunchInputs& in);            // validates, builds the decoded float atlas when a LUT needs it, fills `in` from the current fields
    // samples first+1 .. first+n of the `n_tiles` tiles of the device list `tiles` in that order (nullptr: the whole frame in raster order), inside the
    // timing window its caller opened, per_launch samples at a time: what prepare_submit returned for the same arguments, after it brought the majorant table, the
    // pool, the workspace and the moments up to date -- outside the window of render() / trace(), which spans the sub-launches alone
    // With clear tiles split off (sky, n_sky: their device list), tiles / n_tiles are the MARCH tiles alone: the pool's allocation sees only those, and every
    // sub-launch's sample window is followed by the sky kernel over the clear ones; the samples of a sub-launch stay what the pool's budget gives the whole tile set, and
    // the rate plan counts all the submit's samples over the time of both kernels (the split moves no sub-launch boundary a caller has sized).  n_tiles == 0 (every tile clear): no pool, no workspace, no path-tracing launch.
    // See-through tiles (n_see) follow the clear ones in `sky` and are treated like them; prepare_submit's n_sky counts both classes.
    int prepare_submit(const LaunchInputs& in, int first, int n, int n_tiles, int n_sky = 0);
    void submit(const LaunchInputs& in, int first, int n, const int32_t* tiles, int n_tiles, int per_launch, const int32_t* sky = nullptr, int n_sky = 0, int n_see = 0);
    void submit_tile_set(const LaunchInputs& in, int first, int n);      // prepare, then one window around a submit over the renderer's tile set (set_tiles), ordered as order_tiles says
    void open_timing_window(hipStream_t s), close_timing_window(hipStream_t s);      // of one call: last_launches, last_kernel_ms, last_pathtrace_ms
    int tile_set_size() const;                 // tiles of the renderer's tile set: the listed ones, or all of the frame
    void unpair_views(SceneParams& P, size_t frame) const;
    int samples_per_launch(const LaunchInputs& in, int n_tiles) const;
    LaunchInputs pending_;
    int pending_n_ = 0, pending_first_ = 0, pending_cap_ = 0;
    void update_majorants(const LaunchInputs& in, BrickGridHIP& g);
    std::vector<int32_t> tiles_host_;
    DeviceBufferPtr tiles_dev_;
    // the launch's own order of those tiles: the costliest first (tile_order; ids empty = the whole frame)
    DeviceBufferPtr order_dev_;
    uint64_t order_key_ = 0;
    std::vector<int32_t> costliest_first(const SceneParams& P, const std::vector<int32_t>& ids, int n_tiles) const;
    const int32_t* tile_order(const SceneParams& P, const std::vector<int32_t>& ids, int n_tiles);
    uint64_t tile_order_key(const SceneParams& P, const std::vector<int32_t>& ids, int n_tiles) const;      // (camera, box, frame size, tile list)
    // The same tiles divided by vr_sky_tiles.h sky_split_tiles3: the march tiles (costliest first if `ordered`, else in the list's order), the clear ones and the
    // see-through ones, as one device list [march | clear | see-through] cached under tile_order's key with `ordered` and with what the see-through class reads
    // besides: the grid frame, the version of the committed volume, the class switch and the uniforms its fallbacks look at.  n_sky + n_see == 0: the list was not
    // built -- the caller launches as without the split.
    struct SplitTiles { const int32_t* march = nullptr; int n_march = 0; const int32_t* sky = nullptr; int n_sky = 0, n_see = 0; };
    SplitTiles split_tiles(const LaunchInputs& in, const std::vector<int32_t>& ids, int n_tiles, bool ordered);
    // the one three-way split of a submit's list: the grid's live cells when the see-through class is on for `in`, the clear tiles alone otherwise
    void split_three(const LaunchInputs& in, const std::vector<int32_t>& ids, int n_tiles, std::vector<int32_t>& march, std::vector<int32_t>& clear, std::vector<int32_t>& see) const;
    DeviceBufferPtr split_dev_;
    uint64_t split_key_ = 0;
    int split_n_sky_ = 0, split_n_see_ = 0;
    uint64_t commit_version_ = 0;              // counts commit(): the live cells a cached split was made from belong to one committed volume
    // adaptive sampling: samples behind each raster tile, meaningful while `sample` == tile_n_sample_ (ragged()); the denoiser's device copy: sized_.tile_n_dev
    std::vector<int32_t> tile_n_;
    int tile_n_sample_ = -1;
    DeviceBufferPtr status_;
    DeviceBufferPtr pool_;
    DeviceBufferPtr workspace_;
    // seed table: the buffer, its capacity and its filled prefix in sample numbers, its key, the stream of the last fill and an event recorded after it
    DeviceBufferPtr seed_table_;
    int seed_cap_ = 0, seed_filled_ = 0, seed_fills_ = 0, seed_budget_mb_ = -1, seed_max_samples_ = 0;      // (the last two: the settings the table was made under)
    int seed_key_[3] = { 0, 0, 0 };                    // (seed, W, H) the entries were hashed for
    bool seed_failed_ = false;                         // an allocation failed: the table stays as large as it is (none: the renderer hashes) until the key or the budget changes
    hipStream_t seed_stream_ = nullptr;
    hipEvent_t seed_event_ = nullptr;
    void drop_seed_table();
    // the table for a launch of the 0-based sample numbers [s0, s0 + n) on `stream`, filled as far as it reaches: *samples = the numbers it covers (0: no table)
    const uint32_t* seed_table_for(const SceneParams& P, int s0, int n, hipStream_t stream, int* samples);
    DeviceBufferPtr stats_;                            // 32 counters of the instrumented kernels (sched_stats)
    // Everything whose contents or validity belong to one frame size W x H: the buffers (each allocated on first use) with the flags that say what they hold.
    // resize() assigns a fresh one, drop_history() a fresh History: a new member needs no line in either.
    struct Sized {
        DeviceBufferPtr features;                      // W*H*8 floats of the last render_features
        int pass = 0, rays = 0;                        // which pass filled it last: 0 none, 1 render_features, 2 render_features_expected with that many rays
        DeviceBufferPtr moments;                       // W*H*4 second moments, allocated by the first launch with `variance` on
        int moments_n = -1;                            // the moments cover samples 1..moments_n (-1: they do not start at sample 1)
        DeviceBufferPtr rs_bg, rs_part, resolved;      // resolve(): B, P and the resolved frame, W*H*4 each
        DeviceBufferPtr ly_split, ly_filtered, layer;  // denoise() with denoise_layers = 1: S, F and the layer L, W*H*4 each (vr_layers.h)
        bool layer_valid = false;                      // `layer` holds the layer of a finished call's merge
        bool layer_guided = false;                     // ... and dn_guide is still that call's: no denoise without layers has overwritten it since (upsample() pairs the two)
        bool layer_gathered = false;                  // ... of a gathered whole frame (part 0 of a ShardedRenderer): the renderer's tile subset is no obstacle to upsample()
        DeviceBufferPtr up_features, up_out, up_layer; // upsample(): the hi feature buffer (W*H*8), the hi frame and the hi layer (W*H*4 each), W x H = up_factor x the frame
        int up_factor = 0;                             // the factor they were allocated and last filled for (0: none)
        DeviceBufferPtr dn_guide, dn_var[2], dn_color[2];  // denoise(): guide W*H*8, variance ping-pong W*H, colour ping-pong W*H*4
        DeviceBufferPtr denoised;                      // W*H*4: the last denoise()'s or denoise_temporal()'s result
        DeviceBufferPtr dn_reject;                     // denoise_temporal() with denoise_reject > 0: the scratch between its two kernels, W*H*8
        bool reject_stat = false;                      // dn_reject holds the statistic of the last denoise_temporal()
        DeviceBufferPtr tile_n_dev, adaptive_lists, adaptive_err;      // adaptive sampling: tile_n_ on the device, the rounds' tile lists and error values
        struct History {                               // denoise_temporal(): a ping-pong pair of
            DeviceBufferPtr color[2], record[2];       // W*H*4 colours and W*H*4 (V, N, K, D) records, and
            DeviceBufferPtr moments[2];                // with denoise_moments = 1 the W*H*4 moment records (m1, m2, E, S); the current half exists iff the history has them
            int cur = -1;                              // the half that holds the history (-1: none)
            bool layers = false;                       // it holds the scattered layer (denoise_layers = 1), not the composite
            bool demod = false;                        // ... divided by the albedo (denoise_demodulate = 1)
            TemporalCamera cam{};                      // the camera of the frame that wrote it
        } hist;
    } sized_;
    void download_whole(const DeviceBufferPtr& b, float* out, const char* absent);      // throws `absent` when b is null; else flushes and copies all of b
    void run_resolve();                                       // resolve()'s launches, after check_resolve
    void set_history_switch(int& field, int v, const char* refusal);      // the body of set_denoise_moments / _resolve / _layers / _filter / _demodulate, each with its own refusal
    DenoiseSigma sigma() const { return { denoise_sigma[0], denoise_sigma[1], denoise_sigma[2], denoise_sigma[3], denoise_sigma[4] }; }      // denoise_sigma as the kernels take it
    DeviceBufferPtr expected_stats_;                   // 4 counters of the last render_features_expected with expected_stats on
    bool expected_stats_valid_ = false;                // ... which that pass filled
    ClearTable clear_table_of(BrickGridHIP& g, const GridView& view, int reach);      // the grid's table of that reach (1 or 2), built on `stream` if it has none
    void check_moments(const char* who);               // throws unless the moments cover samples 1..sample (of every tile, on a ragged frame)
    void run_denoise(const char* who, bool temporal, bool whole_frame_gathered = false);  // the body of both; whole_frame_gathered: part 0 of a ShardedRenderer,
                                                       // whose moments and features hold every part's tiles (gather_guides) -- the tile subset is no obstacle then
    friend struct ShardedRenderer;                     // sharded.h: packs sized_.moments / features of every part, unpacks into part 0's, runs part 0's filter
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    std::vector<hipEvent_t> pt_events_;                // (begin, end) around the path-tracing kernel of every sub-launch
    size_t pt_events_used_ = 0;
    double last_ms_ = 0.0, last_pathtrace_ms_ = 0.0;
    bool timing_pending_ = false;
    // launch sizing: samples per millisecond of the last finished path-tracing sub-launch, and a fingerprint of the settings it ran with
    double rate_samples_per_ms_ = 0.0;
    uint64_t rate_key_ = 0, rate_pending_key_ = 0;
    double rate_pending_samples_ = 0.0;               // samples of the last sub-launch enqueued (its events: the last pair of pt_events_)
    void harvest_rate(bool wait);
    MajKey maj_key_;
};

using Renderer = RendererHIP;

}  // namespace vr
