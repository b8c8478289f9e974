/*
 * volren_amd.h -- C ABI of libvolren_amd.so, the MI355X (gfx950, HIP) drop-in for the offline path-tracing path of
 * nihofm/volren.
 *
 * The reference exposes this path as an in-process C++ object API (struct RendererOpenGL, class Environment,
 * class TransferFunction) that is bound to Python by pybind11 (src/bindings.cpp:64-209).  This header is the same
 * surface flattened to C so that any FFI (ctypes, cgo, JNI, N-API, or a pybind11 module like the reference's
 * `volpy`) can bind it: plain pointers and sizes, int return codes (0 = ok, non-zero = the std::runtime_error the
 * C++ method threw; text via vr_last_error()).  Each entry point names the reference interface it replaces
 * (paths relative to the reference repository).  INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions kept from the reference: framebuffers are RGBA32F with row 0 at the BOTTOM (GL image order); matrices
 * are column-major (glm); `sample` counts completed samples per pixel; the running mean of
 * shader/pathtracer_brick.glsl:36 is what the framebuffer holds.
 *
 * There is no CPU path: every compute entry point fails with VR_ERR_NO_DEVICE when no HIP device is present.
 */
#ifndef VOLREN_AMD_H
#define VOLREN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_OK 0
#define VR_ERR 1              /* std::runtime_error / std::out_of_range from the C++ layer */
#define VR_ERR_NO_DEVICE 2
#define VR_ERR_ARG 3

typedef struct vr_renderer vr_renderer;

/* text of the last error on this thread ("" if none) */
const char* vr_last_error(void);
/* library version string */
const char* vr_version(void);
/* number of HIP devices visible (does not initialise a device context) */
int vr_device_count(void);

/* --- lifetime: std::make_shared<RendererOpenGL>() + RendererOpenGL::init()  (src/main.cpp:445-446, src/renderer.cpp:29-50)
 *     device: HIP device ordinal; width/height: Context::resolution() (src/renderer.cpp:47) */
int vr_create(vr_renderer** out, int device, int width, int height);
void vr_destroy(vr_renderer* r);
/* RendererOpenGL::resize (src/renderer.cpp:52-54); clears the framebuffer */
int vr_resize(vr_renderer* r, int width, int height);

/* --- scene loading: load_volume / load_envmap / load_transferfunc of src/main.cpp:37-81 (same side effects:
 *     load_volume sets density_scale=1, scale_and_move_to_unit_cube(), commit(), sample=0; load_envmap resets
 *     transform/strength; load_transferfunc sets show_environment=false) */
int vr_load_volume(vr_renderer* r, const char* path);              /* .brick / .dense / .raw file, or a folder of such frames */
int vr_load_envmap(vr_renderer* r, const char* path);              /* Radiance .hdr */
/* `renderer.volume = Volume(path)` of the pybind11 module (src/bindings.cpp:82,176): replaces the volume and nothing else --
 * no density_scale reset, no unit cube, no commit; the caller runs vr_scale_and_move_to_unit_cube() / vr_commit() in the
 * reference's order (scripts/datagen_colmap.py:57-63, datagen_denoise.py:85-86) */
int vr_set_volume_path(vr_renderer* r, const char* path);
/* voldata::Volume::AABB(name) / minorant_majorant(name) (src/bindings.cpp:91,93; used by scripts/datagen_*.py to place the
 * camera): world-space box, out = min xyz, max xyz */
int vr_volume_aabb(vr_renderer* r, const char* name, float out[6]);
int vr_volume_minorant_majorant(vr_renderer* r, const char* name, float out[2]);
int vr_load_transferfunc(vr_renderer* r, const char* path);        /* "%f, %f, %f, %f" rows */

/* --- scene from memory: voldata::DenseGrid(w,h,d,float*) + Volume(grid) (src/main.cpp:470-472, bindings.cpp Volume ctors);
 *     transform: grid index->model, 16 floats column-major (NULL = identity).  name: "density" | "temperature" | "flame" | "flames".
 *     unit_cube != 0 applies load_volume's density_scale=1 + scale_and_move_to_unit_cube().  Follow with vr_commit(). */
int vr_set_volume_dense(vr_renderer* r, const char* name, const float* voxels, int nx, int ny, int nz, const float* transform, int unit_cube);
/* voldata::Volume::add_grid_frame / update_grid_frame / n_grid_frames (src/bindings.cpp:89-90; voldata is not vendored: call sites
 * src/main.cpp:47, src/renderer.cpp:61-75): append an animation frame holding the dense float grid `name`, or replace grid `name` of frame
 * `frame`.  Follow with vr_commit(); select the frame to render with vr_set_int "grid_frame_counter". */
int vr_volume_add_grid_frame_dense(vr_renderer* r, const char* name, const float* voxels, int nx, int ny, int nz, const float* transform);
int vr_volume_update_grid_frame_dense(vr_renderer* r, int frame, const char* name, const float* voxels, int nx, int ny, int nz, const float* transform);
int vr_volume_n_grid_frames(vr_renderer* r, int* n);
/* dense fp16 grid that STAYS dense on the device (no brick conversion; north_star "dense fp16 grid"): voxels are IEEE
 * binary16, x fastest.  No reference counterpart (the reference bricks every grid in commit(), src/renderer.cpp:63). */
int vr_set_volume_dense_f16(vr_renderer* r, const char* name, const uint16_t* voxels, int nx, int ny, int nz, const float* transform, int unit_cube);
/* voldata::BrickGrid fields as stored in a .brick file; mips may be NULL/0 */
int vr_set_volume_brick(vr_renderer* r, const char* name, const float* transform, const uint32_t n_bricks[3], const float min_maj[2],
                        const uint32_t* indirection, const uint32_t* range, const uint32_t atlas_dim[3], const uint8_t* atlas,
                        int n_mips, const uint32_t* const* mips, const uint32_t (*mip_dims)[3], int unit_cube);
/* Environment(Texture2D) (src/environment.cpp:11-33): float RGB, rows top first */
int vr_set_envmap(vr_renderer* r, const float* rgb, int width, int height);
/* TransferFunction(std::vector<glm::vec4>) (src/transferfunc.cpp:19-22); n = 0 removes the transfer function */
int vr_set_transferfunc(vr_renderer* r, const float* rgba, int n);

/* --- public fields of RendererOpenGL / Environment / TransferFunction / camera (src/renderer.h:30-62, environment.h:20-21,
 *     transferfunc.h:39, src/main.cpp:360-435).  Names: "sample" "sppx" "seed" "bounces" "show_environment" "tonemapping"
 *     "gpu_encoder" (dense grids are bricked on the device, default 1)
 *     "integrator" (0 DDA tracking = both reference kernels, 1 global-majorant tracking = common.glsl:333-394, 2 direct volume rendering
 *     = common.glsl:571-591, needs a transfer function, 3 trace_path around the 64-step ray-marching trackers = common.glsl:506-566)
 *     "variance" (default 0; 1 = every accumulation pass also keeps the per-pixel second moments of the samples: vr_variance)
 *     "denoise_iterations" (a-trous iterations of vr_denoise, 0 .. 10, default 5; 0 = the colour unchanged)
 *     "fast_math" (0 = the specified, bit-reproducible arithmetic; 1 = opt-in tolerance mode: hardware log/sin/cos/rcp, within 1e-3
 *     relative L2 of the default -- refused with VR_ERR while a transfer function is bound, where it misses that bound)
 *     "tf_float_atlas" (default 1: transfer-function renders of brick grids decode the atlas to floats once, 4x its size; 0 = read the bytes)
 *     "grid_frame_counter"
 *     "sample_pool_mb" (HBM budget of the per-sample radiance pool, 16 .. 65536, default 65536: allocated only as large as a launch needs)
 *     "seed_table_mb" (HBM budget of the renderer's path-seed table, 0 .. 8192, 0 = no table, -1 = back to the default min(4096, "sample_pool_mb" / 4), which
 *     vr_get_int reports as that number.  A new path's RNG state is a 32-round hash of (seed, width, pixel, sample number) only; the renderer keeps the hashes of
 *     the whole frame's first samples, 4 bytes per pixel of the 16x16-tile grid and sample, and the path-tracing kernel reads them instead of hashing.  The table is
 *     keyed by (seed, width, height): vr_reset keeps it, a change of one of the three drops it; it grows to the samples the launches have asked for, up to the
 *     budget, and the samples beyond are hashed as before, as are all samples of scenes whose kernel is no faster with the table (dense grids, emission grids,
 *     "kernel_variant" != 0: their launches make none).  A table that cannot be allocated is given up with one note on stderr: no render fails for it.  The parts
 *     of a sharded renderer hold a table each, indexed by the whole frame's tiles, so parts that share a device cover the same samples once per part.
 *     Results never depend on the table)
 *     "seed_table_max_samples" (default 0 = as many samples per pixel as "seed_table_mb" holds; > 0: at most this many, the samples beyond hash in the kernel)
 *     "launch_target_ms" (default 2000: a vr_render is split into sub-launches planned to take at most this long each, from the rate this
 *     renderer measured last -- a short probe launch, one synchronisation, when it has none for the current settings and the request is
 *     large; 0 = split by the sample pool alone.  Results never depend on the split)
 *     "order_tiles" (a launch works through its tiles costliest first -- longest chord of the pixel rays through the volume's box -- so that short
 *     paths are what is left when its work queue runs empty: 0 = never (raster order), 1 = when a tile subset is set (vr_set_tiles / a sharded
 *     renderer's parts; default), 2 = always.  Results never depend on the order)
 *     "sky_tiles" (0 / 1, default 1.  A 16x16 tile is CLEAR when no camera ray of any of its pixels, for any jitter, can hit the volume's box: its pixel
 *     rectangle, grown by one pixel on every side, lies apart from the projection of the box's eight corners, all of them in front of the camera -- decided on
 *     the host from camera, box and frame size alone; no tile is clear with the camera inside the box or a corner behind or near the camera plane.  Every sample of
 *     a clear tile is the environment behind it (black with "show_environment" 0), alpha 0.  With 1 those tiles are rendered by one thread per pixel and the
 *     path tracer and its sample pool see only the others; "order_tiles" orders those.  Where a vr_render is cut into sub-launches ("sample_pool_mb",
 *     "launch_target_ms") does not move: both go on counting every tile.  A view without clear tiles is launched exactly as with 0.  The split is OFF, whatever the value, while vr_sched_stats counts (every sample passes through the instrumented kernels), with "fast_math" 1 and
 *     with "integrator" 2 or 3.  Results never depend on it: the frames are the same bits.  A camera ray of a clear tile that does hit the box -- a bug of the
 *     classification -- is reported by vr_synchronize like a tripped watchdog, in words of its own)
 *     "see_through_tiles" (0 / 1, default 1.  A tile is SEE-THROUGH when rays of it surely cross the box (its rectangle, SHRUNK by one pixel, meets the box's projection) and no camera ray of its pixels can come within reach of a density tap
 *     of an 8^3-voxel cell of the density grid whose range allows density > 0: its rays cross the box, but no real collision can happen on them, so every sample
 *     of it is the environment, alpha 0, as well.  Decided on the host from the grid's range table -- every live cell grown by 3.5 voxels, projected, its
 *     rectangle grown by one pixel.  Where "sky_tiles" splits a submit, such tiles go to the same per-pixel kernel, without its box test.  None for "integrator"
 *     other than 0 or 1, with an emission grid or a transfer function bound, a density scale that is negative or not finite, the camera inside the box, a live
 *     cell behind or beside the camera, a NaN in the range table, or a float grid (encoded on the device: the host holds no table).  Results never depend on it)
 *     (int);  "tonemap_exposure" "tonemap_gamma" "albedo"(3) "phase" "density_scale"
 *     "emission_scale" "vol_clip_min"(3) "vol_clip_max"(3) "env_strength" "env_transform"(9) "env_rot"(1, degrees about +y,
 *     main.cpp:382) "tf_window_left" "tf_window_width" "cam_pos"(3) "cam_dir"(3) "cam_up"(3) "cam_fov" "volume_transform"(16)
 *     "denoise_sigma"(5: the edge-stopping widths of vr_denoise for colour, normal, depth, coverage, albedo; each in [2^-60, 2^60], about
 *     [8.7e-19, 1.15e18]: VR_ERR otherwise, the old values kept; default 4, 0.5, 0.1, 0.25, 0.2) (float) */
/* read-only through vr_get_int: "last_sky_tiles" (the clear tiles of the last submit -- the last vr_render / flushed vr_trace run, or the last group of a
 *     vr_render_adaptive: what "sky_tiles" kept out of the path tracer there; 0 when that submit was not split) and "last_see_through_tiles" (the same for the
 *     see-through tiles; "last_sky_tiles" counts the clear ones only);  "seed_table_samples" (samples 1 .. this of every pixel have their seeds in the table now; 0 = no table) and "seed_table_fills"
 *     (fill launches of this renderer so far: a frame that repeats the last one's seed, size and samples adds none);  "kernel_variant" (the compiled path-tracing kernel the next launch uses: 0 brick grid, 1 dense fp16 grid, 2 / 4 brick grid +
 *     emission grid, 3 everything decided at run time -- correct for every scene, up to an order of magnitude slower) and "kernel_variant_reason" (what sent the
 *     scene to variant 3, a mask: 1 integrator != 0, 2 the environment's warp table has thresholds below 2^-76 ("env_div_safe" = 0), 4 density scale outside
 *     [2^-16, 2^24], 8 emission grid with a dense grid / brick grids of different layouts; 0: the scene has a kernel of its own kind).  Reasons 2 and 4 are also
 *     said once per process on stderr: a caller cannot see them coming;  "env_compact" (1: every texel of the environment map is exactly an RGBE number -- a
 *     Radiance file's always are -- and the path tracer fetches them as one dword each; the values are the float map's, bit for bit);  "kernel_wide" (1: the next
 *     launch's path-tracing kernel forms 64-bit gather addresses -- a grid table of 4 GiB or more, kernel variants 2 to 4, or "wide_addressing" -- 0: 32-bit byte
 *     offsets from the tables' bases).  Diagnostic, through vr_set_int: "wide_addressing" (default 0 = by the tables' sizes; 1 = always the 64-bit kernels.  Same results) */
int vr_set_int(vr_renderer* r, const char* name, int value);
int vr_get_int(vr_renderer* r, const char* name, int* value);
int vr_set_float(vr_renderer* r, const char* name, const float* values, int count);
int vr_get_float(vr_renderer* r, const char* name, float* values, int count);

/* RendererOpenGL::commit / reset / scale_and_move_to_unit_cube (src/renderer.cpp:56-76,155-157,227-242) */
int vr_commit(vr_renderer* r);
int vr_reset(vr_renderer* r);
int vr_scale_and_move_to_unit_cube(vr_renderer* r);

/* --- the hot path.  vr_trace = RendererOpenGL::trace (src/renderer.cpp:78-145): ONE more sample per pixel.
 *     vr_render = the Python binding's render(spp) loop (src/bindings.cpp:124-132) / the offline loop (src/main.cpp:533-537)
 *     fused into one launch: `spp` more samples per pixel (spp <= 0: up to sppx).  Both are asynchronous on the renderer's
 *     stream; vr_synchronize waits and reports a tripped kernel watchdog as an error.
 *     The reference's own loop `while (sample < sppx) trace();` runs at vr_render's speed (round 5): a vr_trace records the launch
 *     inputs it found ("sample" advances by one, invalid state is reported at the call) and consecutive calls that find the same
 *     bytes are launched TOGETHER -- at the next call of this header that could observe or change the frame (vr_synchronize,
 *     vr_framebuffer*, vr_draw / vr_display / vr_save_png, vr_render, vr_commit, vr_resize, vr_set_tiles, vr_pack_tiles /
 *     vr_unpack_tiles, vr_set_stream, vr_last_*_ms, vr_sched_stats), at a vr_trace that finds changed inputs (any vr_set_*
 *     in between: the recorded samples are launched with the values they were recorded with, as the reference's already issued
 *     dispatches are), or when a full sub-launch has been recorded.  vr_flush launches what has been recorded without waiting;
 *     vr_set_int "coalesce_trace" 0 makes every vr_trace its own launch again; vr_get_int "pending_samples" reads the count. */
int vr_trace(vr_renderer* r);
int vr_flush(vr_renderer* r);
int vr_render(vr_renderer* r, int spp);
int vr_synchronize(vr_renderer* r);
/* duration of the last path-tracing launch in ms, measured with HIP events on the renderer's stream (waits for it) */
int vr_last_kernel_ms(vr_renderer* r, double* ms);
/* duration of the path-tracing kernel alone, summed over the sub-launches of the last vr_trace / vr_render (without the accumulation
 * passes); 0 if that call launched none (integrators 2 and 3 run their own kernels) */
int vr_last_pathtrace_ms(vr_renderer* r, double* ms);

/* --- results.  vr_framebuffer = fbo_data() without the alpha drop (src/bindings.cpp:141-148): W*H*4 floats, row 0 bottom.
 *     vr_draw = RendererOpenGL::draw (src/renderer.cpp:147-153) into a separate tonemapped buffer (shader/tonemap.glsl);
 *     vr_save_png = tonemap + Texture2D::save_ldr of the offline loop (src/main.cpp:540-555): RGBA8 PNG, top row first. */
int vr_framebuffer(vr_renderer* r, float* rgba_out);
int vr_framebuffer_device(vr_renderer* r, void** device_ptr);
/* --- denoiser data (no reference counterpart; the reference's scripts/datagen_denoise.py exports colour only).
 *     vr_render_features: for every pixel of the tile set, the first scattering event of colour samples 1..spp -- same seed, jitter and camera
 *     ray as colour sample s, then the first segment of the DDA tracker (common.glsl:458-501) with the same draws, whatever "integrator" is and
 *     always in the specified arithmetic ("fast_math" does not apply).  Per pixel, over the samples that collide (H of spp): albedo (vol_albedo
 *     [x the LUT's rgb]), normal (-normalize(transpose(Minv3) g), g the central difference of the trilinear density, not renormalised after
 *     averaging) and depth (distance along the unit camera ray) averaged, and coverage = H / spp; zeros where H = 0.  Not progressive: each call
 *     computes samples 1..spp afresh.  Asynchronous on the renderer's stream; a flush point like vr_render.  Bounded like the path tracer: a
 *     segment whose ray parameter can no longer advance (a camera very far from the volume for its voxel size) ends without a collision, and
 *     a pixel whose segment exceeds a step budget stops there, which the next vr_synchronize reports as an error.
 *     vr_render_features_expected fills the same buffer with the EXPECTED VALUES of those features instead of a sample mean: per pixel rays x rays
 *     deterministic sub-rays (rays in 1..4, else VR_ERR_ARG; sub-ray (i, j) takes the jitters ((i + 0.5) / rays, (j + 0.5) / rays) in the camera
 *     expression above), each marched through the volume's box in m = clamp(ceil(length in voxels), 1, 4096) equal steps of length h.  A step at
 *     its midpoint t looks up the trilinear density, sigma = density_scale x it (with a LUT: sigma = LUT alpha x majorant, albedo x LUT rgb), and
 *     weighs w = T (1 - exp(-sigma h)), T *= exp(-sigma h), until T <= 2^-10; the normal is -normalize(transpose(Minv3) g) with g the analytic
 *     gradient of the trilinear interpolant.  With K = sum w: albedo = sum(w a) / K, coverage = K / rays^2, normal = sum(w n) / K, depth =
 *     sum(w t) / K, zeros where K = 0 -- the limit of vr_render_features for spp -> infinity (without a LUT up to the tracker's smoother
 *     stochastic-tricubic field), free of noise, independent of "seed", "integrator" and the emission grid, and bit-identical from call to call
 *     under the same camera and scene.  All in float32 as volren_amd/csrc/vr_expected.h states it.  Asynchronous on the renderer's stream and a
 *     flush point like vr_render_features; it counts as a feature pass for every call that needs one, and every reader of the feature buffer
 *     (vr_features, vr_denoise, vr_denoise_temporal, vr_sharded_gather_guides, vr_render_adaptive's frames) reads it unchanged.  Bounded by
 *     construction (at most 16 x 4096 steps per pixel): it never sets the status word.
 *     Empty space: with vr_set_int "expected_skip" 1 (the default; 0 = every step runs; other values VR_ERR) the march reads a clear-distance table
 *     of the density grid -- one byte per cell of 8^3 voxels (the bricks; ceil(dim / 8) cells per axis of a dense grid): 0 when some voxel of the
 *     cell's box grown by one voxel does not decode to +0.0f, else min(255, Chebyshev distance in cells to the nearest such cell) -- and drops, with
 *     their eight loads, the steps whose midpoint lies in a cell with a byte >= 1, leaping 7 (byte - 1) further steps where a step is at most a
 *     voxel long (volren_amd/csrc/vr_clear.h, vr_expected.h).  Results never depend on the setting: a dropped step is one that adds nothing.  Under
 *     a LUT whose alpha at density 0 is positive empty space is not empty and every step runs.  The table (2 MiB for 1024^3 voxels) is built on the
 *     device by the first such pass after the grid was committed, once per frame of an animation; renders that never ask for the pass pay nothing.
 *     The default is 1 for every grid kind: on no measured scene was 1 slower than 0 (profiles/r12_expected_skip.txt).
 *     vr_set_int "expected_stats" 1 (default 0) makes the following passes count their work in an instrumented twin of the kernel; vr_expected_stats
 *     waits and writes the last pass's totals: out[0] sub-rays marched, [1] steps reached (dropped ones included), [2] steps that fetched their
 *     corners, [3] reads of the table; VR_ERR when "expected_stats" was off for that pass.  vr_expected_clear_table (test hook) writes the table of
 *     the current density grid, built if need be, x fastest, and its extent in cells; out may be NULL (the extent alone).
 *     The field: vr_set_int "expected_field" 0 (the default) marches the trilinear density as above; 1 marches the field the path tracer decides
 *     its collisions on (other values VR_ERR).  Without a transfer function that is the separable cubic B-spline of the voxels -- the mean of the
 *     tracker's stochastic tricubic tap: 64 taps a step, floor(p - 0.5) - 1 .. + 2 per axis, value and gradient from the same taps
 *     (volren_amd/csrc/vr_cubic.h) -- and the coverage is then the one the framebuffer's alpha converges to: the trilinear march lies 4e-4 below it
 *     on smoke.brick and 6e-3 on a dense 64^3 grid, the cubic one within sampling noise at 4096 spp.  With a transfer function the tracker itself
 *     looks up the trilinear field, and 1 gives the same bits as 0.  The cubic march skips empty space by a table of its own, of reach 2 (the
 *     cell's box grown by two voxels, 12^3), built and cached like the other; vr_expected_clear_table returns the table the current setting marches
 *     with, and the frame is the same bits with "expected_skip" 0 and 1.  It costs 3 to 4 times the trilinear pass, and 2 x 2 cubic rays cost more
 *     than the 16-spp stochastic pass (profiles/r22_expected_cubic.txt).  The setting acts on every expected-value pass -- tile subsets, the parts
 *     of a sharded renderer, vr_upsample's pass at the large size -- and changing it drops no temporal history: the next pass is simply another
 *     guide.
 *     vr_features waits and writes W*H*8 floats (albedo.rgb, coverage, normal.xyz, depth), row 0 at the bottom; VR_ERR before the first
 *     vr_render_features since the last resize.
 *     vr_variance waits and writes W*H*4 floats: the unbiased per-channel variance of the samples 1..n behind the framebuffer (0 for n = 1),
 *     kept when vr_set_int "variance" is 1 (default 0; the buffer is allocated only then).  VR_ERR unless "variance" was on for every one of
 *     samples 1..n (switched on mid-frame: vr_reset and render again). */
int vr_render_features(vr_renderer* r, int spp);
int vr_render_features_expected(vr_renderer* r, int rays);
int vr_expected_stats(vr_renderer* r, uint64_t out[4]);
int vr_expected_clear_table(vr_renderer* r, uint8_t* out, int cells[3]);
int vr_features(vr_renderer* r, float* out);
int vr_variance(vr_renderer* r, float* rgba_out);
/* --- denoiser (no reference counterpart either: scripts/datagen_denoise.py exports the noisy colour for a denoiser of the caller's own).
 *     vr_denoise: the edge-avoiding a-trous wavelet filter (the spatial part of SVGF, Schied et al. 2017) of the current frame, guided by the
 *     per-pixel variance and the last vr_render_features: "denoise_iterations" passes at steps 1, 2, 4, ... of a 5x5 B3-spline kernel whose taps are
 *     weighted down by differences in luminance (relative to the filtered standard deviation), coverage, normal, depth and albedo ("denoise_sigma";
 *     the arithmetic is specified operation by operation in volren_amd/csrc/vr_denoise.h and reproducible bit for bit).  Asynchronous on the
 *     renderer's stream; a flush point like vr_render_features.  VR_ERR when no feature pass has run since the last resize, when "variance" was not
 *     on for every one of samples 1..n, when n < 1, or while a tile subset is set (the filter reads neighbours: whole frames only).  The framebuffer,
 *     the moments, the features and what vr_draw / vr_display / vr_save_png show are left as they were.
 *     vr_denoised waits and writes W*H*4 floats, linear (not tonemapped), row 0 at the bottom; VR_ERR before the first vr_denoise since the last
 *     resize. */
int vr_denoise(vr_renderer* r);
int vr_denoised(vr_renderer* r, float* rgba_out);
/* --- temporal accumulation in front of the filter (no reference counterpart; the temporal part of SVGF, reprojected by depth).
 *     vr_denoise_temporal: as vr_denoise -- the same inputs, the same refusals, whatever vr_denoise accepts -- but the frame is first blended into a
 *     history of the frames before it, and the filter starts from the blended colour and variance.  The history of a pixel is read where the pixel's
 *     first-scatter point (the centre ray at the guide's depth; the ray's direction where the pixel shows the environment only) lay on the screen
 *     of the call before, from up to four bilinear taps that pass a coverage and depth test (relative depth difference <= 0.1); a pixel without such a
 *     tap starts afresh.  While "cam_pos", the camera's orientation and "cam_fov" are what they were at the call before, every pixel reads its own
 *     history, unresampled.  Blend: N = min(N + 1, 2^20) frames behind the pixel, a = max("denoise_alpha", 1 / N), C = (1 - a) history + a frame,
 *     V = (1 - a)^2 V_history + a^2 v.  The arithmetic is specified operation by operation in volren_amd/csrc/vr_temporal.h and reproducible bit for bit.
 *     Call it once per frame (a second call on the same frame blends the frame with itself), on frames of equal samples per pixel: the blend
 *     treats frames as equals.  Meant for fixed cameras (animations, progressive refinement) and slow camera paths; see README.md for where it stops paying.
 *     The history is created by the first call, dropped by vr_resize and vr_denoise_history_reset, and KEPT across vr_reset, vr_set_*, the loaders and
 *     vr_commit: a sequence is reset, render, render_features, denoise_temporal per frame, and what no longer matches is for the depth and coverage test
 *     to reject.  vr_denoise neither reads nor writes it.  A device allocation that fails makes the call fail and leaves the last result and the history
 *     as they were.  The first call gives what vr_denoise gives.  vr_denoised returns the result of whichever of the two calls ran last.
 *     vr_denoise_history waits and writes the history: the blended colour (W*H*4), the blended variance of the mean's luminance (W*H) and the number of
 *     frames behind each pixel (W*H), row 0 at the bottom; any pointer may be NULL; VR_ERR while there is no history.
 *     vr_set_float / vr_get_float "denoise_alpha"(1: the smallest weight of the current frame, in [2^-20, 1]: VR_ERR otherwise, the old value kept;
 *     default 0.1).
 *     History rejection, off by default.  The tests above compare what a pixel shows, never its colour: after a change of the lighting or of the volume
 *     the history lags by 1 / "denoise_alpha" frames.  vr_set_float / vr_get_float "denoise_reject"(1: the threshold tau; 0 = off, the default, and then
 *     every launch and result is what it is without this paragraph; otherwise in [2^-10, 2^20]: anything else, NaN included, is VR_ERR, the old value
 *     kept).  With tau > 0 a pixel with a history forms z2 = (luma(history) - luma(frame))^2 / (V_history + v + 1e-12), whose expectation is 1 while
 *     nothing changed, and T = the mean of z2 over the pixels of its 5x5 neighbourhood that lie in the frame and have a history; unless T <= tau
 *     (a NaN fails) the pixel starts afresh like one without a history: C = frame, V = v, N = 1.  3 is a good tau: under 1 % of the pixels of an unchanged
 *     scene.  Two limits: the frames need n >= 2 samples per pixel (with n = 1 the variance v is 0 and whatever changed at all is rejected), and the floor
 *     1e-12 assumes radiances far above 1e-6.  Costs one scratch buffer of W*H*8 floats, allocated like the others before anything is launched.
 *     vr_denoise_reject_stat waits and writes W*H floats, row 0 at the bottom: T of the last vr_denoise_temporal, -1 where the pixel had no history;
 *     VR_ERR unless the last vr_denoise_temporal since the resize ran with "denoise_reject" > 0.
 *     Luminance moments, off by default.  The filter's variance above is the frames' sample variance, which a frame of one sample per pixel does not
 *     have: at 1 spp v = 0, vr_denoise is the identity and vr_denoise_temporal a bare running mean.  vr_set_int / vr_get_int "denoise_moments" (0 or 1;
 *     default 0, and then every launch, allocation and result is what it is without this paragraph; anything else is VR_ERR, the old value kept; a
 *     call that changes the value drops the history: one without moment records cannot continue one with them).  With 1 the history carries a
 *     third array, W*H*4 floats (m1, m2, E, S): the integrated first and second moments of the frame's luminance L (m1 = (1 - a) m1_history + a L,
 *     m2 likewise from L^2, fetched from the same taps as the colour), E = (1 - a)^2 E_history + a^2 the sum of squared blend weights (1 without a
 *     history), and S the variance of one frame's luminance: m2 - m1^2 (not below 0) where N >= 4 frames lie behind the pixel, and where fewer do --
 *     the first frames, disoccluded pixels -- the same from m1, m2 averaged over the 7x7 neighbourhood with the filter's coverage, normal, depth and
 *     albedo weights.  The filter starts from V = S E, and the frame's own v is not used.  The arithmetic is specified operation by operation in
 *     volren_amd/csrc/vr_moments.h and reproducible bit for bit.  Use it for sequences of 1 to a few samples per pixel (previews, fly-throughs): at
 *     1 spp it takes the error of the first frame to 0.42 and that of frames 10 to 15 to 0.56 of the running mean's (README.md); from 2 spp on the
 *     sample variance is as good, and better during the first three frames, hence a setting.  The refusals stay what they are ("variance" = 1 for
 *     every sample included).  With "denoise_moments" = 1 and "denoise_reject" > 0 vr_denoise_temporal is VR_ERR, nothing is launched and the last
 *     result and the history stay as they were: one-sample luminances are too heavy-tailed for the rejection statistic.
 *     vr_denoise_history_moments waits and writes W*H*4 floats (m1, m2, E, S), row 0 at the bottom; VR_ERR unless the current history was written with
 *     "denoise_moments" = 1. */
int vr_denoise_temporal(vr_renderer* r);
int vr_denoise_history_reset(vr_renderer* r);
int vr_denoise_history(vr_renderer* r, float* rgba_out, float* var_out, float* length_out);
int vr_denoise_reject_stat(vr_renderer* r, float* out);
int vr_denoise_history_moments(vr_renderer* r, float* out);
/* --- the frame's hit/miss noise replaced by the expected coverage: a control variate in image space (no reference counterpart).
 *     A sample's alpha is 1 when its path scattered at least once and 0 when it flew through, so the framebuffer's alpha is kappa^, the share of a
 *     pixel's samples that hit.  vr_render_features_expected gives the same number without noise: kappa, the coverage channel of the feature buffer.
 *     In a partially covered pixel a sample is either the environment behind the volume (radiance B) or scattered light (conditional mean C); which
 *     of the two is a coin toss whose variance kappa (1 - kappa) (B - C)^2 dominates the pixel wherever the environment is much brighter or darker
 *     than the volume.  vr_resolve removes it:
 *         y = x + beta (kappa^ - kappa),   beta = B - C~
 *     x the frame's mean; B the mean environment radiance over the sub-rays of the expected pass (what the path tracer adds for an escaping camera
 *     ray, strength and transform included; 0 while "show_environment" is 0); C~ = sum (x - (1 - kappa^) B) / sum kappa^ over the pixel's 7x7
 *     neighbourhood, 0 where nothing in it hit; y.rgb not below 0, y.a = kappa.  A pixel with kappa^ = kappa keeps its rgb bit for bit.  The arithmetic
 *     is specified operation by operation in volren_amd/csrc/vr_resolve.h and reproducible bit for bit.
 *     Expectation: E[y] = E[x] + beta (E[kappa^] - kappa).  Under a transfer function the path tracer's tracker collides on the very field the expected
 *     pass marches, and y is unbiased up to the coupling of C~ with kappa^.  Without one the tracker uses the smoother stochastic-tricubic field: the
 *     two coverages differ by about 0.002 on average, and y carries beta times that as bias (README.md states the measured bias and the sample count
 *     up to which the call pays).  With an emission grid the estimator stays valid but beta is no longer the best coefficient.
 *     vr_resolve: asynchronous on the renderer's stream; a flush point like vr_denoise.  Works at any sample count, on ragged frames of
 *     vr_render_adaptive too (only means are used), and needs no "variance".  VR_ERR, before anything is launched, when no sample is in the frame,
 *     while a tile subset is set, while "integrator" is 2 (its alpha is an opacity, not a hit indicator), when the feature buffer was not last filled
 *     by vr_render_features_expected since the last resize, or when that pass ran with rays < 2 (one ray gives the coverage of the pixel's centre,
 *     not of its area).  The framebuffer, the features, the moments and what vr_draw / vr_display / vr_save_png show are left as they were; the three
 *     W*H*4 buffers of the call are allocated by the first call and dropped by vr_resize.
 *     vr_resolved waits and writes W*H*4 floats, linear (not tonemapped), row 0 at the bottom; vr_resolve_background (a test hook) the same of B, alpha 0.
 *     Both are VR_ERR before the first vr_resolve since the last resize.
 *     vr_set_int / vr_get_int "denoise_resolve" (0 or 1; default 0, and then every launch, allocation and result is what it is without this
 *     paragraph; anything else is VR_ERR, the old value kept; a call that changes the value drops the history).  With 1, vr_denoise and
 *     vr_denoise_temporal -- with "denoise_reject" and with "denoise_moments" too -- run vr_resolve first and start from y instead of the
 *     framebuffer's colour, with the frame's variance unchanged (a variance derived for y filtered worse); whatever vr_resolve refuses they refuse
 *     then, besides their own refusals.  vr_sharded_denoise / vr_sharded_denoise_temporal honour part 0's setting: part 0 holds the gathered frame and
 *     guide, the resolve runs there, and the result is bit for bit one device's. */
int vr_resolve(vr_renderer* r);
int vr_resolved(vr_renderer* r, float* rgba_out);
int vr_resolve_background(vr_renderer* r, float* rgba_out);
/* --- the filter on the scattered layer alone, normalised by the expected coverage (no reference counterpart).
 *     A partially covered pixel shows (1 - kappa) B + kappa C.  kappa is exact (vr_render_features_expected), B analytic (vr_resolve); only C is noisy.
 *     vr_set_int / vr_get_int "denoise_layers" (0 or 1; default 0, and then every launch, allocation and result is what it is without this
 *     paragraph; anything else is VR_ERR, the old value kept; a call that changes the value drops the history).  With 1, vr_denoise and
 *     vr_denoise_temporal -- with "denoise_reject" and with "denoise_moments" too -- run vr_resolve's kernels (whatever "denoise_resolve" says), then
 *         split:   G = (1 - kappa) B;   S.rgb = y.rgb - G (signed);   S.a = kappa
 *         filter:  their own kernels, unchanged, on S in place of the frame, with the frame's variance: F (F.a is kappa under the colour's weights)
 *         merge:   L.rgb = F.a > 2^-20 ? F.rgb * (kappa / F.a) : F.rgb;   L.a = kappa;   out.rgb = max(0, G + L.rgb);   out.a = kappa
 *     so the sky seen through thin smoke is not blurred and the silhouette ramp is kappa's own; a pixel with kappa = 0 within the filter's reach of
 *     the volume (F.a > 2^-20) comes out as B bit for bit.
 *     The arithmetic is specified operation by operation in volren_amd/csrc/vr_layers.h and reproducible bit for bit.  vr_denoised returns out;
 *     under vr_denoise_temporal the history (vr_denoise_history) holds the layer S blended over the frames, not the composite, so a turning camera
 *     does not drag old sky along behind the volume.  Whatever vr_resolve refuses these calls refuse then, before anything is launched, besides their
 *     own refusals: it needs vr_render_features_expected with rays >= 2 as the last feature pass.  Without a transfer function kappa lies about
 *     0.0004 below the path tracer's coverage, and that bias stays, as with vr_resolve, unless "expected_field" is 1.  README.md has the measured errors, among them the case that
 *     loses.  vr_sharded_denoise / vr_sharded_denoise_temporal honour part 0's setting, bit for bit one device's result.
 *     vr_denoised_layer waits and writes L of the last such call, W*H*4 floats, linear, row 0 at the bottom: the scattered light premultiplied by the
 *     exact coverage, alpha = kappa; composite it over any background B' as (1 - a) B' + rgb.  VR_ERR before the first vr_denoise or
 *     vr_denoise_temporal with the setting on since the last resize.
 *     The filter of the layer: vr_set_int / vr_get_int "denoise_filter" (0 or 1; default 0, and then every launch, allocation and result is what it is
 *     without this paragraph; anything else is VR_ERR, the old value kept; a call that changes the value drops the history).  With 1 -- and
 *     "denoise_layers" = 1: without it vr_denoise and vr_denoise_temporal are VR_ERR before anything is launched, as they are for whatever "denoise_layers"
 *     itself refuses -- one pass of weighted local regression over an 11 x 11 window takes the place of the a-trous iterations; the resolve, the split,
 *     the temporal blend with rejection or moments and the merge stay as they are, and "denoise_iterations" = 0 still leaves S unfiltered.  Per pixel p
 *     with kappa_p > 0, over the taps q with S_q.a > 2^-20 and kappa_q > 0 (dy outer, dx inner):
 *         w = s(dx) s(dy) e_q S_q.a,  s the Gaussian of sigma 2.5, e_q = w_n w_d w_a of vr_denoise with "denoise_sigma" (1 at the centre, and 1 unless both
 *             coverages are positive); no colour weight, no coverage weight, and the variance is neither read nor written
 *         x = (1, (d_q - d_p) / max(d_p, 2^-20), n_q - n_p, a_q - a_p): the fit C ~ beta . x of the targets S_q.rgb / S_q.a by weighted least squares, with
 *             lambda sum(w) added to the seven slopes' diagonal, lambda = vr_set_float "denoise_ridge" (0, or in [2^-20, 2^20]; VR_ERR otherwise)
 *         F.rgb = kappa_p beta_0, F.a = kappa_p; lambda = 0 is zero order, beta_0 = sum(w c) / sum(w), and the default (README.md has the sweep that chose it)
 *     and F = 0 where kappa_p = 0 or sum(w) <= 2^-20, so every pixel without coverage comes out as B bit for bit.  The arithmetic is specified operation
 *     by operation in volren_amd/csrc/vr_regress.h and reproducible bit for bit; vr_upsample, the history and vr_sharded_denoise (part 0's settings) take
 *     it as they take the a-trous's result.
 *     Albedo demodulation: vr_set_int / vr_get_int "denoise_demodulate" (0 or 1; default 0, and then every launch, allocation and result is what it is
 *     without this paragraph; anything else is VR_ERR, the old value kept; a call that changes the value drops the history).  Every scattered sample is
 *     a_1 R, the first collision's albedo times everything after it; under a transfer function a_1 holds the colour texture and R is smooth, and the
 *     expected-value pass gives the pixel's mean a_1 without noise (words 0..2 of the feature buffer).  With 1 -- and "denoise_layers" = 1: without it
 *     vr_denoise and vr_denoise_temporal are VR_ERR before anything is launched -- per pixel and channel
 *         d = kappa > 0 ? max(albedo, 2^-6) : 1
 *         S.rgb = (y.rgb - G) / d, and the variance the filter reads is that of the divided layer: (sum_c w_c sqrt(var_c) / d_c)^2 / n
 *         the filter ("denoise_filter" 0 or 1), the temporal blend with rejection or moments and the history: unchanged, on the divided layer
 *         L.rgb = (the merge's L.rgb) d;  out.rgb = max(G + L.rgb, 0)
 *     so vr_denoised_layer keeps its meaning, and a pixel with kappa = 0 comes out as it does without the setting, bit for bit.  vr_upsample with the setting
 *     1 at its call divides every lo texel by the d of the lo guide before its taps and multiplies the hi layer by the d of the hi guide, whatever produced
 *     the lo layer.  A channel whose albedo lies below the floor keeps at most 2^-6 of its neighbours' irradiance as bias; light that carries no a_1 (an
 *     emission grid's) is divided all the same, amplified by at most 64 before the filter.  With the setting on, a wide "denoise_sigma" albedo value (README.md
 *     has the tables) lets the filter cross the colour edges that d has taken out: a gain for frames of a few spp, a loss at 64.  The arithmetic is specified operation by operation in
 *     volren_amd/csrc/vr_demod.h and reproducible bit for bit; vr_sharded_denoise takes part 0's setting. */
int vr_denoised_layer(vr_renderer* r, float* rgba_out);
/* --- the denoised scattered layer upsampled under a full-resolution guide (no reference counterpart).
 *     kappa and B of (1 - kappa) B + kappa C are functions of the camera ray alone and cost no path-tracing sample at any resolution; C is smooth after the
 *     filter.  So a frame can be path-traced and filtered `factor` times smaller per axis -- the same samples buy factor^2 times the spp there -- and the
 *     full-size picture rebuilt from its layer.  vr_upsample(r, factor, rays), after vr_denoise or vr_denoise_temporal with "denoise_layers" = 1 on the
 *     renderer's w x h frame ("lo"), writes the W = factor w by H = factor h frame ("hi") into buffers of its own:
 *         guide:   an expected-value pass of rays x rays sub-rays at W x H (bit for bit vr_render_features_expected's of a renderer resized to W x H; it honours
 *                  "expected_skip" and "expected_stats" alike), and B_p, vr_resolve's background, at W x H
 *         taps:    the 4 x 4 lo pixels around the hi pixel's centre, spatial weight s the uniform cubic B-spline's, edge factor e = w_n w_d w_a of vr_denoise
 *                  between the hi and the lo guide with "denoise_sigma" (1 unless both coverages are positive); no colour and no coverage weight
 *         C = sum (s e) L_q.rgb / sum (s e) kappa_q where that sum exceeds 2^-20, else the same with s alone, else 0
 *         L_p.rgb = kappa_p C;   L_p.a = kappa_p;   out.rgb = max(0, (1 - kappa_p) B_p + L_p.rgb);   out.a = kappa_p
 *     so the silhouette ramp and the sky are the hi frame's own, and a hi pixel with kappa_p = 0 is B_p bit for bit.  The arithmetic is specified operation
 *     by operation in volren_amd/csrc/vr_upsample.h and reproducible bit for bit.  Asynchronous on the renderer's stream, and a flush point like vr_denoise.
 *     VR_ERR_ARG for a factor outside 2..4 or rays outside 1..4.  VR_ERR, before anything is launched, when vr_denoised_layer would be refused (no denoise call
 *     with "denoise_layers" = 1 since the last resize) or a tile subset is set; and, with words of its own ("the last denoise ran with denoise_layers = 0"),
 *     when the last vr_denoise / vr_denoise_temporal that ran did so with "denoise_layers" = 0: the lo guide is the one that call prepared, so it no longer
 *     belongs to the layer -- vr_denoised_layer stays readable, vr_upsampled* keep what they held, and a call with "denoise_layers" = 1 makes vr_upsample
 *     available again (a refused denoise call changes nothing of this).  The first call allocates the hi buffers; vr_resize drops them, and so does a
 *     call with another factor.  The hi guide is marched when the call is made: the camera and the scene are the caller's to keep as they were at the denoise
 *     call.  The framebuffer, vr_features, vr_denoised, vr_denoised_layer and the history are left as they were.  There is no history at the hi size.
 *     Sharded renderers: after vr_sharded_denoise part 0 holds the gathered frame, guide and layer, and vr_upsample on vr_sharded_part(s, 0) is the call -- one
 *     device's work.  README.md has the measured errors and costs, among them the cells that lose.
 *     vr_upsampled and vr_upsampled_layer wait and write W*H*4 floats, linear, row 0 at the bottom: out, and L (premultiplied by the exact coverage, alpha =
 *     kappa_p; composite it as (1 - a) B' + rgb).  vr_upsampled_features writes the hi feature buffer, W*H*8 floats in vr_features' layout.  vr_upsampled_size
 *     writes (W, H).  All four are VR_ERR before the first vr_upsample since the last resize. */
int vr_upsample(vr_renderer* r, int factor, int rays);
int vr_upsampled(vr_renderer* r, float* rgba_out);
int vr_upsampled_layer(vr_renderer* r, float* rgba_out);
int vr_upsampled_features(vr_renderer* r, float* out);
int vr_upsampled_size(vr_renderer* r, int wh[2]);
/* --- adaptive sampling (no reference counterpart): "render until the error is below t, at most N spp", decided per 16x16 tile.
 *     The error of tile t is e_t, the worst relative standard error of a pixel mean's luminance in the tile: per pixel of n samples,
 *     e_p = sqrt(the variance of the mean's luminance, as vr_denoise forms it) / (luma(mean) + 2^-10), +inf for n < 2; e_t = the max over the
 *     tile's pixels inside the frame (NaN if any e_p is).  The arithmetic is specified in volren_amd/csrc/vr_adaptive.h and reproducible bit for bit.
 *     vr_render_adaptive: the tiles of the tile set (vr_set_tiles; none = every tile) below min_spp are brought to min_spp; then, while some
 *     tile of the set has fewer than max_spp samples, one round evaluates e_t of those tiles, retires the ones with e_t < threshold (strict: a
 *     threshold of 0 never retires a tile) and takes each other tile from n_t to min(2 n_t, max_spp) samples.  It starts from the uniform frame
 *     of "sample" samples or from the counts a previous call left, keeps the per-pixel moments for all its launches whatever "variance" says
 *     (the setting is left as it was) and ends with "sample" = the largest count of any tile.  A tile brought to k samples is bit for bit the
 *     tile of a k-spp vr_render, moments included.  Asynchronous like vr_render, except that each round waits for its error values (one small
 *     copy) and reports a tripped watchdog as vr_synchronize would; vr_get_int "adaptive_rounds" counts the rounds of the last call.
 *     VR_ERR when "sample" > 0 and the moments do not cover samples 1..sample ("variance" off for some of them: vr_reset and render again).
 *     vr_tile_samples / vr_tile_error wait and write one value per raster tile of the frame (t = ty * ceil(W/16) + tx, row 0 = bottom).
 *     Ragged frames: a call that leaves tiles at different counts leaves a "ragged" frame.  While "sample" keeps the value that call left:
 *     vr_trace and vr_render refuse it (VR_ERR, frame untouched: vr_reset, or continue with vr_render_adaptive), vr_variance applies each
 *     tile's own n / (n - 1) (0 for n < 2), vr_denoise takes each tile's own n (VR_ERR if a tile holds no samples), and vr_last_kernel_ms /
 *     vr_last_pathtrace_ms cover the whole vr_render_adaptive call: all its launches, and the sum of all its path-tracing kernels.  Anything
 *     that changes "sample" ends the ragged state (vr_reset, vr_resize, the loaders, vr_set_int "sample" -- even to the same value): the frame
 *     counts as uniform again.  A call that ends with every tile at one count leaves an ordinary uniform frame.
 *     Bias: the decision to stop uses the variance estimated from the very samples it judges, so tiles whose estimate came out low stop early
 *     and the result is biased towards them -- as in the adaptive samplers of production renderers; there is no second sample buffer here.
 *     A tile whose pixels saw no collision in its first min_spp samples (the volume is thin there) has zero estimated variance and retires at
 *     once: keep min_spp at 16 or more.  Not available on the sharded renderer (the parts would end at different "sample" values). */
/* render until every tile of the tile set has e_t < threshold or max_spp samples (the schedule above); 2 <= min_spp <= max_spp,
   threshold finite and >= 0, else VR_ERR_ARG; VR_ERR for missing moments or a tripped watchdog */
int vr_render_adaptive(vr_renderer* r, int min_spp, int max_spp, float threshold);
/* samples behind each raster tile (row 0 = bottom, t = ty * ceil(W/16) + tx); a uniform frame gives `sample` everywhere;
   n_tiles must be ceil(W/16) * ceil(H/16) (VR_ERR_ARG otherwise); waits */
int vr_tile_samples(vr_renderer* r, int32_t* out, int n_tiles);
/* e_t of every tile at its current count (same kernel as the schedule); needs the moments to cover the frame; waits */
int vr_tile_error(vr_renderer* r, float* out, int n_tiles);
int vr_draw(vr_renderer* r);
int vr_display(vr_renderer* r, float* rgba_out);
int vr_save_png(vr_renderer* r, const char* path);

/* --- additions for multi-GPU and measurement (no reference counterpart) */
/* restrict rendering to these 16x16 tiles (raster tile ids, row 0 = bottom); n = 0 -> whole frame */
int vr_set_tiles(vr_renderer* r, const int32_t* tile_ids, int n);
/* use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream */
int vr_set_stream(vr_renderer* r, void* hip_stream);
/* pack the owned tiles of the framebuffer into a compact device buffer (n_tiles*256*4 floats) / scatter a gathered buffer back */
int vr_pack_tiles(vr_renderer* r, const int32_t* tile_ids_device, int n_tiles, void* packed_device);
int vr_unpack_tiles(vr_renderer* r, const int32_t* tile_ids_device, int n_tiles, const void* packed_device);
/* --- ONE frame on SEVERAL devices, in one process (no reference counterpart: the reference drives one GL context, src/main.cpp:524-557;
 *     SURVEY.md 8e; volren_amd/csrc/sharded.h).  vr_sharded_create makes n_parts renderers, part i on HIP device devices[i] (vr_create each).
 *     The scene is REPLICATED by the caller: apply the scene calls of this header (vr_load_volume, vr_set_float, ...) to every
 *     vr_sharded_part(s, i).  vr_sharded_render deals the frame's 16x16 tiles diagonally (owner = (tx + ty) mod n_parts), lets every part
 *     render `spp` more samples of its tiles on its own stream, and gathers the accumulated radiance with ONE collective per frame
 *     (RCCL over xGMI; librccl.so.1 is opened at run time): grouped ncclSend / ncclRecv to part 0 ("gather", the default: only part 0 needs -- and
 *     allocates -- the whole frame), or a grouped ncclAllGather with VR_SHARDED_COLLECTIVE=allgather (rounds 4-5); vr_sharded_collective says which; afterwards part 0's framebuffer (vr_framebuffer / vr_save_png on
 *     vr_sharded_part(s, 0)) holds the whole frame, bit-identical to a single-device render.  Parts that share a device (logical shards:
 *     devices = {0, 0, 0}) exchange their tiles with device-to-device copies instead -- vr_sharded_transport says which: "rccl", "copy", or
 *     "none" for one part; environment VR_SHARDED_TRANSPORT=copy|rccl overrides (rccl also with ONE part: a one-rank communicator).
 *     Asynchronous like vr_render; vr_sharded_synchronize waits for every part and reports a tripped watchdog.  The parts belong to the
 *     sharded renderer: never vr_destroy one, never vr_set_stream / vr_set_tiles on one.
 *     Denoising: set "variance" to 1 on every part before the frame's first sample.  vr_sharded_render_features runs vr_render_features(spp) on every
 *     part that owns tiles, over its tiles, on its own stream (no exchange).  vr_sharded_gather_guides packs every part's per-pixel moments and
 *     features of its own tiles (three float4 per pixel), moves them to part 0 in ONE exchange on the transport above (3x the colour's size; its
 *     buffers are allocated by the first call, a caller that only renders pays nothing) and scatters them into part 0's moments and features.
 *     vr_sharded_denoise / vr_sharded_denoise_temporal do that and then run vr_denoise / vr_denoise_temporal's filter on part 0 over the whole frame,
 *     with part 0's "denoise_iterations", "denoise_sigma", "denoise_alpha", "denoise_reject", "denoise_moments" and camera: bit-identical to the single-device calls.  Results are read
 *     from part 0: vr_denoised, vr_features, vr_variance (both after a gather), vr_denoise_history, vr_denoise_history_moments and vr_denoise_reject_stat on vr_sharded_part(s, 0); the temporal history lives
 *     in part 0 and vr_denoise_history_reset on part 0 drops it.  All three are asynchronous, and a sequence reset, render, render_features, denoise per
 *     frame needs no synchronisation between frames.  VR_ERR, before anything is launched and with a message that names the part, unless all parts agree
 *     on the resolution and "sample", "sample" >= 1, and every part that owns tiles has moments that cover samples 1..n, a feature pass since the last
 *     resize and no ragged frame; the last result and the history are then left as they were.  vr_denoise on a part itself keeps refusing the part's
 *     tile subset, and vr_render_adaptive stays a single-device call.  Like the colour gather, the guide exchange has run between logical shards of
 *     one device and on a one-rank communicator only. */
typedef struct vr_sharded vr_sharded;
int vr_sharded_create(vr_sharded** out, const int* devices, int n_parts, int width, int height);
void vr_sharded_destroy(vr_sharded* s);
int vr_sharded_parts(vr_sharded* s);
vr_renderer* vr_sharded_part(vr_sharded* s, int i);
const char* vr_sharded_transport(vr_sharded* s);
const char* vr_sharded_collective(vr_sharded* s);         /* "gather" | "allgather": what the rccl transport runs per frame */
int vr_sharded_reset(vr_sharded* s);                      /* vr_reset on every part */
int vr_sharded_render(vr_sharded* s, int spp);
int vr_sharded_render_features(vr_sharded* s, int spp);   /* spp >= 1, as vr_render_features */
int vr_sharded_render_features_expected(vr_sharded* s, int rays);   /* rays in 1..4: vr_render_features_expected on every part that owns tiles, over its tiles */
int vr_sharded_gather_guides(vr_sharded* s);
int vr_sharded_denoise(vr_sharded* s);
int vr_sharded_denoise_temporal(vr_sharded* s);
int vr_sharded_synchronize(vr_sharded* s);
/* the tile deal itself (host only, needs no device): owner_out[t] = the part (0 .. n_parts-1) that renders raster tile t of a width x height frame,
 * t = ty * ceil(width / 16) + tx, row 0 = bottom; n_tiles must be ceil(width / 16) * ceil(height / 16) */
int vr_tile_owners(int width, int height, int n_parts, int32_t* owner_out, int n_tiles);
/* the seed table's arithmetic (host only, needs no device): the default "seed_table_mb" of a renderer whose "sample_pool_mb" is sample_pool_mb, and the
 * samples per pixel a budget of mb MiB covers on a width x height frame (4 bytes x 256 x ceil(width / 16) x ceil(height / 16) per sample) */
int vr_seed_table_default_mb(int sample_pool_mb);
int vr_seed_table_samples_for(int mb, int width, int height);
/* the uniform block the next launch would use (struct vr::Uniforms of volren_amd/csrc/vr_scene.h, `bytes` must match) */
int vr_get_uniforms(vr_renderer* r, void* out, int bytes);
int vr_uniforms_size(void);
/* importance pyramid of the current environment (floats, level 0 first); count from vr_impmap_floats */
int vr_impmap_floats(vr_renderer* r);
int vr_get_impmap(vr_renderer* r, float* out, int count);
/* scheduler thresholds of THIS renderer's path-tracing launches (8 ints, vr::PathtraceTuning::thr in volren_amd/csrc/vr_device.h);
 * tuning state is per renderer: two renderers in one process, on one device or two, never share it */
int vr_set_sched(vr_renderer* r, const int32_t thresholds[8]);
/* FNV-1a checksums of the committed density grid's device arrays: [0] brick records, [1] atlas, [2] range words (tests: the
 * device encoder and the host encoder must agree) */
int vr_grid_checksums(vr_renderer* r, uint64_t out[3]);
/* scheduler statistics of this renderer's launches (diagnostics): enable != 0 starts counting (instrumented kernels); out (32 x uint64,
 * may be NULL) receives, per state, [block executions, active lanes], then [16] wave iterations, [17] waves, [18..24] cycles per
 * state, [25] summed wave lifetime, [26..31] summed pool occupancy */
int vr_sched_stats(vr_renderer* r, int enable, unsigned long long* out);
/* diagnostics: after an instrumented launch (vr_sched_stats enable), out[3 i .. 3 i + 2] = when wavefront i started, found the work queue empty and ended
 * (ticks of the device's constant 100 MHz clock; 0 = no such wavefront); n_words <= 3 * 8192 */
int vr_wave_timeline(vr_renderer* r, unsigned long long* out, int n_words);
/* test hook: device allocations above `mb` MiB fail as if the device were out of memory (the fall-back paths can then be exercised on a
 * shared GPU); mb < 0 removes the cap.  Initial value: environment variable VR_TEST_MAX_ALLOC_MB, read once per process. */
int vr_test_alloc_cap_mb(long long mb);
/* unit-test probe of the device math (volren_amd/csrc/vr_math.h): host arrays in/out */
int vr_math_probe(int fn, const float* a, const float* b, float* out, int n);
/* test hook: the same probe over a range of bit patterns, out[i] = f(bits(first + i), b) (first + i wraps modulo 2^32); one launch, count <= 2^26.
 * fn: volren_amd/csrc/vr_math_probe.h (17 has no sweep form); 100..103: the tolerance-mode forms of neg_log_1m (of the draw (first + i) 2^-24), sincos_ (sine, cosine), unorm8 (of (first + i) & 255) */
int vr_math_sweep(int fn, uint32_t first, long long count, float b, float* out);
/* test hook: unit-test probe of the scene-data lookups (volren_amd/csrc/vr_probe.h): n items of probe `what` (0 voxel, 1 trilinear, 2 majorant, 3 importance,
 * 4 texel, 5 sky, 6 light sample, 7 transfer function, 8 cubic B-spline lookup: value and gradient) in compile-time form `form`, on the scene as the renderer's next
 * launch would read it.  in: 4 32-bit words per item; out: 1, 1, 1, 1, 3, 3, 7, 4, 4 floats per item; host arrays.  VR_ERR_RUNTIME for a form the scene cannot serve (the message says why). */
int vr_probe(vr_renderer* r, int what, int form, const void* in, float* out, long long n);
/* test hook: unit-test probe of the per-path layer (volren_amd/csrc/vr_path_probe.h): n items of `kind` (0 RNG, 1 camera ray, 2 box clip, 3 phase function and
 * MIS weight, 4 DDA step, 5 one whole segment of the hot pair, bounded) in form `form` (DDA step: 0 general, 1 CLEAN; segment: the compiled instance 0..6), on the
 * scene as the renderer's next launch would read it.  in: 8, 4, 6, 9, 7, 8 32-bit words per item; out: 5, 4, 3, 5, 1, 14 32-bit words per item (floats as their bits);
 * host arrays, at most 2^24 items.  VR_ERR_RUNTIME for a form the scene cannot serve -- an instance the scene's launch would not run -- with the reason. */
int vr_path_probe(vr_renderer* r, int kind, int form, const void* in, void* out, long long n);
/* test hook: ONE launcher of the image-space kernels (volren_amd/csrc/vr_device.h, section vr_filters.hip) on host arrays of the caller's.  The arrays of
 * `in` go up into fresh device buffers, the stage's launch_* runs once on the renderer's stream, the call waits, and the arrays of `out` come back.  No buffer,
 * flag or history of the renderer changes; the renderer gives its device and stream, and to the two scene-bound stages (resolve, upsample) its scene.
 * W x H: the frame (upsample: the LO frame; the outputs are f W x f H).  in: 6 pointers, out: 5 pointers, NULL where the stage has none or an optional one is
 * left out; params: 40 floats -- [0..4] sigma (colour, normal, depth, coverage, albedo), [5] an integer i0, [6] a float x, [7] tau, [8] an integer i1,
 * [9..21] the current camera, [22..34] the history's (pos 3, cam_transform 9 column-major, cam_z), [35] an integer demod, the rest 0.  float arrays of 4 bytes, counts and ids int32.
 *   stage                 launcher                 in                                                            params               out
 *   0 prepare             launch_denoise_prepare   moments S W*H*4, features W*H*8, [counts, one per tile]       i0 = n, x = vscale   v W*H, guide W*H*8
 *   1 atrous              launch_denoise_atrous    colour W*H*4, v W*H, guide W*H*8                              i0 = step, sigma     colour W*H*4, [v W*H]
 *   2 temporal            launch_denoise_temporal  colour, v, guide, [hist colour W*H*4, hist record W*H*4,      x = alpha, tau,      colour, record W*H*4 each, v W*H,
 *                                                  [hist moments W*H*4]]                                         i1 = same_cam, both  [moments W*H*4], [scratch W*H*4 =
 *                                                                                                                cameras, sigma       (T, N_h, z2, has)]
 *       out[3] set: the moments form (vr_moments.h; in[5] with a history); tau > 0: the rejection form, out[4] must be set; else the plain pass
 *   3 resolve             launch_resolve           fb W*H*4, features W*H*8                                      i0 = rays            B, Pq, out W*H*4 each
 *   4 split               launch_layers_split      y W*H*4, B W*H*4, features W*H*8                                                   S W*H*4
 *   5 merge               launch_layers_merge      F W*H*4, B W*H*4, features W*H*8                                                   out, L W*H*4 each
 *   6 regress             launch_denoise_regress   S W*H*4, guide W*H*8                                          x = ridge, sigma     F W*H*4
 *   7 upsample            launch_upsample          lo layer W*H*4, lo guide W*H*8, hi features fW*fH*8           i0 = rays, i1 = f,   out, L fW*fH*4 each
 *                                                                                                                sigma
 *   8 adaptive error      launch_adaptive_error    fb W*H*4, moments W*H*4, tile ids i0, counts i0               i0 = the tiles       e_t i0
 * demod (0 or 1; default 0, and then every launch is what it is without this line): 1 runs the stage's DEMOD instance ("denoise_demodulate" = 1,
 * volren_amd/csrc/vr_demod.h) in stages 0, 4, 5 and 7, which read the albedo in words 0..2 of their features (7: of the lo guide and of the hi features).
 * Stages 3 and 7 read the scene as the renderer's next launch would (7: with the resolution f W x f H, as vr_upsample forms it) and need W x H to be the
 * renderer's resolution.  Everything that can be checked without a device is checked before the device is looked for: VR_ERR_ARG for a NULL renderer or array,
 * an unknown stage, W, H outside 1..4096, step outside 1..2^20, rays outside 1..4, f outside 2..4, n < 1, a tile id outside the frame, tau < 0, a parameter
 * that is not finite, a demod other than 0 or 1, demod = 1 at a stage other than 0, 4, 5 or 7, the moments and the rejection form together, a history given in part; and, with a device, for a W x H that is not the renderer's in stages 3 and 7.
 * The values INSIDE the arrays are the caller's business: tests/filter_cases.py holds the catalogue the suite runs (frames of 64 x 48 at most, built to the edges
 * of what the product's own passes can hand these kernels), and every case of it passes the host build of its stage, range-checked, in
 * tests/test_filter_cases_host.py before tests/test_gpu_filter_probe.py runs it on a device. */
#define VR_FILTER_PROBE_IN 6
#define VR_FILTER_PROBE_OUT 5
#define VR_FILTER_PROBE_PARAMS 40
int vr_filter_probe(vr_renderer* r, int stage, int W, int H, const void* const* in, float* const* out, const float* params);
/* voldata::Volume::to_brick_grid + BrickGrid serialisation: encode a dense float grid (x fastest) and write it as a .brick
 * container (SURVEY.md 2.3 layout); transform may be NULL (identity).  Host only, needs no device. */
int vr_write_brick_from_dense(const float* voxels, int nx, int ny, int nz, const float* transform, const char* path);
/* writes this build's ".dense" container (the serialized dense grid main.cpp:44 can load; voldata's own layout is not
 * vendored): u8 voxels, x fastest, value = lo + u8 / 255 * (hi - lo) */
int vr_write_dense(const uint8_t* voxels, int nx, int ny, int nz, float lo, float hi, const float* transform, const char* path);
/* host-side helpers exposed for tests: dense->brick encoder statistics */
int vr_encode_dense_stats(const float* voxels, int nx, int ny, int nz, uint32_t n_bricks_out[3], uint64_t* brick_counter, float min_maj_out[2]);

#ifdef __cplusplus
}
#endif
#endif /* VOLREN_AMD_H */
