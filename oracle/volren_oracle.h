/*
 * oracle/volren_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement (plain C) of nihofm/volren's ray-marching hot path
 * (shader/pathtracer_brick*.glsl + shader/common.glsl) and of the host steps on
 * either side of it (src/renderer.cpp, src/environment.cpp, src/transferfunc.cpp,
 * shader/env_setup.glsl, shader/tonemap.glsl).  Every function cites the reference
 * file:line it follows.
 *
 * PARITY PINNED AGAINST OUTPUTS OF THE REFERENCE ITSELF, RUN HERE.  The reference has no
 * tests or golden vectors and its host program cannot be built (cppgl/voldata are not
 * vendored), but its hot path is GLSL, and Mesa's software rasteriser is in the image:
 * oracle/glref runs the reference's own shader files (read from /root/reference/shader)
 * on llvmpipe, tests/golden/make_golden_glsl.py stores the outputs (tests/golden/
 * glsl_golden.npz) and tests/test_glsl_pin.py checks this oracle against them: whole
 * renders (path tracer with and without transfer function, emission) to ~1e-7 relative L2
 * for the unfused build of this file (llvmpipe never fuses multiply-add), >= 99.5 % of
 * the pixels to 1e-5 for the standard build; tea/rng, majorant fetches and a complete
 * transmittanceDDA segment bit for bit.  In addition: structural known-answers on the
 * reference's data files (tests/golden/known_answers.json) and the reference's only
 * output artefact imgs/example.jpg (tests/golden/example_64.npy).  DESIGN.md 2 has the
 * details, including the three points GLSL/GL leave to the driver (precision of
 * log/acos/atan, multiply-add contraction, the generic GL_COMPRESSED_RED atlas format).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library.  The product (volren_amd/) never includes, links or calls it.
 */
#ifndef VOLREN_ORACLE_H
#define VOLREN_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* voldata::BrickGrid as stored in a .brick file */
typedef struct {
    float    transform[16];     /* glm::mat4, column-major */
    uint32_t n_bricks[3];
    float    min_maj[2];
    uint64_t brick_counter;
    uint32_t* indirection;      /* n_bricks.x*y*z words, GL_RGB10_A2UI packing */
    uint32_t* range;            /* 2 x fp16: low half = min, high half = max */
    uint32_t atlas_dim[3];
    uint8_t* atlas;
    uint32_t n_mips;
    uint32_t mip_dim[8][3];
    uint32_t* mips[8];          /* range mip levels 1..n_mips */
    /* build-only extension (no reference counterpart): dense fp16 voxels [z][y][x] instead of indirection+atlas
     * (north_star "dense fp16 grid"); extent = voxel dimensions (0 -> n_bricks*8 as for a loaded BrickGrid) */
    uint32_t extent[3];
    const uint16_t* dense;
} orc_brickgrid;

/* the uniform block RendererOpenGL::trace uploads (src/renderer.cpp:88-138) */
typedef struct {
    int32_t bounces, seed, show_environment;
    float cam_pos[3], cam_fov, cam_transform[9];
    float vol_bb_min[3], vol_bb_max[3];
    float vol_minorant, vol_majorant, vol_inv_majorant;
    float vol_albedo[3], vol_phase_g, vol_density_scale, vol_emission_scale, vol_emission_norm;
    float vol_density_transform[16], vol_density_inv_transform[16];
    float vol_emission_transform[16], vol_emission_inv_transform[16];
    uint32_t tf_size; float tf_window_left, tf_window_width;
    float env_transform[9], env_inv_transform[9], env_strength, env_imp_inv_dim[2];
    int32_t env_imp_base_mip;
    int32_t resolution[2];
    /* build-only switches */
    int32_t use_tf;          /* pathtracer_brick_tf.glsl vs pathtracer_brick.glsl */
    int32_t has_emission;    /* emission grid bound (renderer.cpp:117-124) */
    int32_t integrator;      /* 0 = USE_DDA (both reference kernels), 1 = global-majorant delta/ratio tracking (common.glsl:333-394),
                              * 2 = direct volume rendering, 64-step ray marcher (common.glsl:571-591; needs a LUT),
                              * 3 = trace_path with the 64-step ray-marching trackers (common.glsl:506-566) */
} orc_params;

typedef struct {
    const orc_brickgrid* density;
    const orc_brickgrid* emission;     /* may be NULL */
    const float* tf_lut;               /* tf_size x 4 (already CDF-fixed), may be NULL */
    const float* envmap;               /* env_w*env_h*3, texture order: row 0 = v~0 (bottom) */
    int32_t env_w, env_h;
    const float* impmap;               /* importance pyramid, level 0 first */
    int32_t imp_dim;                   /* 512 */
} orc_scene;

/* per-sample event counters for SURVEY 8(d)'s algorithmic-bytes formula */
typedef struct {
    uint64_t samples;
    uint64_t n_dda_sv, n_dda_tr;       /* DDA loop iterations in sample_volumeDDA / transmittanceDDA */
    uint64_t n_coll_sv, n_coll_tr;     /* tentative collisions */
    uint64_t n_nee;                    /* real scatter events (NEE evaluations) */
    uint64_t n_esc;                    /* escaped paths that fetch the environment */
    uint64_t n_primary_miss;           /* camera rays that miss the clip box */
    uint64_t n_tf_lookup;              /* tf_lookup calls (on-chip traffic) */
    uint64_t n_ended;                  /* paths that end with free_path == 0: the bounce cap or the roulette (samples - n_ended leave the volume) */
} orc_counters;

/* ---- loaders ---- */
int  orc_load_brick(const char* path, orc_brickgrid* out);           /* 0 ok */
void orc_free_brick(orc_brickgrid* g);
/* Radiance RGBE -> float RGB, rows in FILE order (top row first) */
int  orc_load_hdr(const char* path, float** rgb, int32_t* w, int32_t* h);
/* LUT text file "%f, %f, %f, %f" per row (src/transferfunc.cpp:79-93); returns rows, -1 on error */
int  orc_load_lut(const char* path, float* rgba, int32_t max_rows);
void orc_free(void* p);

/* ---- host steps ---- */
/* TransferFunction::upload_gpu + compute_lut_cdf (src/transferfunc.cpp:33-58); in place; returns 1 if the CDF fix-up ran */
int  orc_lut_fixup(float* rgba, int32_t n);
/* flip rows so that row 0 = bottom (texture order) */
void orc_flip_rows(float* rgb, int32_t w, int32_t h, int32_t ch);
/* Environment ctor: env_setup.glsl + glGenerateMipmap (src/environment.cpp:11-33); out has orc_impmap_floats(dim) floats */
int32_t orc_impmap_floats(int32_t dim);
void orc_build_impmap(const float* env_tex, int32_t w, int32_t h, int32_t dim, float* out);
/* bilinear envmap fetch used everywhere (GL_LINEAR, repeat u, clamp v) */
void orc_env_texture(const float* env_tex, int32_t w, int32_t h, float u, float v, float rgb[3]);

/* RendererOpenGL::scale_and_move_to_unit_cube (src/renderer.cpp:227-242): volume_transform out, density_scale in/out */
void orc_unit_cube(const orc_brickgrid* g, float volume_transform[16], float* density_scale);
/* camera: cam_transform = inverse(mat3(lookAt(pos,pos+dir,up))) (src/renderer.cpp:95) */
void orc_camera(const float pos[3], const float dir[3], const float up[3], float cam_transform[9]);
/* glm::mat3(glm::rotate(mat4(1), radians(deg), (0,1,0))) (src/main.cpp:382) */
void orc_env_rotation(float deg, float m[9]);
/* fills the volume/grid dependent uniforms exactly like RendererOpenGL::trace (src/renderer.cpp:96-124) */
void orc_volume_uniforms(orc_params* p, const orc_brickgrid* density, const orc_brickgrid* emission,
                         const float volume_transform[16], float density_scale,
                         const float clip_min[3], const float clip_max[3], float majorant_emission);
void orc_mat3_inverse(const float m[9], float out[9]);
void orc_mat4_inverse(const float m[16], float out[16]);
void orc_mat4_mul(const float a[16], const float b[16], float out[16]);

/* ---- the hot path ---- */
/* Runs samples first_sample..first_sample+n_samples-1 (1-based, like current_sample) for the pixel rectangle
 * [x0,x1) x [y0,y1) of a W x H image and applies the running-mean update of pathtracer_brick.glsl:36 to
 * fb (RGBA32F, W*H*4, row 0 = bottom).  threads <= 0 -> all cores.  counters may be NULL. */
void orc_render(const orc_params* p, const orc_scene* s, float* fb,
                int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                int32_t first_sample, int32_t n_samples, int32_t threads, orc_counters* counters);

/* one path, for unit tests: returns vec4(L, alpha) of trace_path for pixel (x,y), sample s */
void orc_trace_pixel_sample(const orc_params* p, const orc_scene* s, int32_t x, int32_t y, int32_t sample, float out[4]);

/* tonemap.glsl:13-36 in place on RGBA32F */
void orc_tonemap(float* fb, int32_t w, int32_t h, float exposure, float gamma);

/* ---- small exports for unit tests ---- */
uint32_t orc_tea(uint32_t v0, uint32_t v1, uint32_t n);
float    orc_rng(uint32_t* state);
float    orc_lookup_density_brick(const orc_brickgrid* g, int32_t x, int32_t y, int32_t z);
float    orc_lookup_majorant_raw(const orc_brickgrid* g, int32_t x, int32_t y, int32_t z, int32_t mip);
void     orc_sample_environment(const orc_params* p, const orc_scene* s, float r0, float r1, float w_i[3], float le_pdf[4]);
void     orc_view_dir(const orc_params* p, int32_t x, int32_t y, int32_t w, int32_t h, float jx, float jy, float out[3]);
int      orc_intersect_box(const orc_params* p, const float pos[3], const float dir[3], float near_far[2]);
int      orc_sample_volume(const orc_params* p, const orc_scene* s, const float pos[3], const float dir[3], uint32_t* seed, float out[4]);
void     orc_sample_phase_hg(const float dir[3], float g, float r0, float r1, float out[3]);
float    orc_phase_hg(float cos_t, float g);
float    orc_transmittance(const orc_params* p, const orc_scene* s, const float pos[3], const float dir[3], uint32_t* seed);
/* batch forms of the lookups (arrays in, arrays out, OpenMP): item i is the four 32-bit words in[4 i ..] -- integers or float bits --
 * voxel: grid (0 density, 1 emission), x, y, z -> lookup_density_brick; trilinear: grid, then the index-space position as float bits ->
 * lookup_density_trilinear (density scale applied); majorant: position as float bits, mip -> the effective lookup_majorant of the DDA
 * trackers (TF-remapped when a LUT is bound); importance: x, y, mip; texel: u, v -> 3 floats; sky: direction -> lookup_environment, 3 floats;
 * light: r0, r1 -> sample_environment as (w_i, Le, pdf), 7 floats, and optionally the base-level texel it ends in; tf: density -> 4 floats */
void     orc_batch_voxel(const orc_scene* s, const uint32_t* in, float* out, int64_t n);
void     orc_batch_trilinear(const orc_params* p, const orc_scene* s, const uint32_t* in, float* out, int64_t n);
void     orc_batch_majorant(const orc_params* p, const orc_scene* s, const uint32_t* in, float* out, int64_t n);
void     orc_batch_importance(const orc_scene* s, const uint32_t* in, float* out, int64_t n);
void     orc_batch_texel(const orc_scene* s, const uint32_t* in, float* out, int64_t n);
void     orc_batch_sky(const orc_params* p, const orc_scene* s, const uint32_t* in, float* out, int64_t n);
void     orc_batch_light(const orc_params* p, const orc_scene* s, const uint32_t* in, float* out, int32_t* texel, int64_t n);
void     orc_batch_tf(const orc_params* p, const orc_scene* s, const uint32_t* in, float* out, int64_t n);

/* Batch forms of the per-path layer (OpenMP over items), for tests/test_path_probes_host.py and tests/test_gpu_path_probes.py: the item layouts of
 * volren_amd/csrc/vr_path_probe.h, 32-bit words in and out (floats as their bits, integers as they are).
 *   rng      in 8: state, v0, v1, seed, W, px, py, smp       out 5: rng(state), state after, state after nine draws, orc_tea(v0, v1, 32), the path seed
 *   camera   in 4: px, py, smp, -                            out 4: pixel_sample's direction (two jitter draws, view_dir), the RNG state after the two draws
 *   box      in 6: pos, dir                                  out 3: hit, near, far
 *   phase    in 9: cos, g, dir, r0, r1, a, b                 out 5: phase_hg(cos, g), sample_phase_hg(dir, g, r0, r1), power_heuristic(a, b)
 *   dda_step in 7: p, 1 / dir, mip                           out 1: stepDDA
 *   segment  in 8: pos, dir, RNG state, kind (0 sample_volume, 1 transmittance), by the tracker p->integrator selects (0 DDA, otherwise the global-majorant
 *            pair), with the loop bounded by ORC_SEGMENT_BUDGET iterations
 *            out 13: status (0 missed the box, 1 the segment ended without a real collision -- kind 1: the ray left the box --, 2 real collision -- kind 1: the
 *            roulette ended the ray --, 3 budget exhausted), t, tau, the DDA level in quarter steps (a ray that misses: 0, 0, 12; the global pair: tau 0, level 12),
 *            the RNG state after, the number of tentative collisions, Tr (kind 0: 1), the colour of the real collision under a LUT (otherwise 0, 0, 0), the
 *            radiance Le gathered with throughput 1 (kind 0 with an emission grid; otherwise 0, 0, 0)
 * The single-item entry points above run the same loops without a bound. */
#define ORC_SEGMENT_BUDGET 4096
void     orc_batch_rng(const uint32_t* in, uint32_t* out, int64_t n);
void     orc_batch_camera(const orc_params* p, const uint32_t* in, uint32_t* out, int64_t n);
void     orc_batch_box(const orc_params* p, const uint32_t* in, uint32_t* out, int64_t n);
void     orc_batch_phase(const uint32_t* in, uint32_t* out, int64_t n);
void     orc_batch_dda_step(const uint32_t* in, uint32_t* out, int64_t n);
void     orc_batch_segment(const orc_params* p, const orc_scene* s, const uint32_t* in, uint32_t* out, int64_t n);
float    orc_math(int32_t fn, float a, float b);   /* 0 log 1 sin 2 cos 3 tan 4 acos 5 atan2 6 exp 7 pow 8 asin */
int32_t  orc_num_threads(void);
/* the product's math probe table (volren_amd/csrc/vr_math_probe.h, codes 0..37 without 12 and 17) from oracle_math.h; operands and results as bit
 * patterns; b may be NULL (0).  The compare forms return the number of elements of got[] that differ from the oracle (floats: any NaN equals any
 * NaN; integer results: never; voxel_index: the property its header states), -1 for an unknown code, and fill bad[24] with
 * (index or input bits, got, want) of the first eight. */
int32_t  orc_math_is_int(int32_t fn);
int32_t  orc_math_known(int32_t fn);
int32_t  orc_math_batch(int32_t fn, const uint32_t* a, const uint32_t* b, uint32_t* out, int64_t n);
int64_t  orc_math_compare(int32_t fn, const uint32_t* a, const uint32_t* b, const uint32_t* got, int64_t n, int64_t* bad);
int64_t  orc_math_sweep_compare(int32_t fn, uint32_t first, int64_t n, uint32_t b, const uint32_t* got, int64_t* bad);

#ifdef __cplusplus
}
#endif
#endif
