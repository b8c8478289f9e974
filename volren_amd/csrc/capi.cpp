// capi.cpp -- extern "C" surface of libvolren_amd.so (include/volren_amd.h) over the C++ classes.
#include "../../include/volren_amd.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <filesystem>
#include <functional>
#include <iostream>
#include <stdexcept>
#include <memory>
#include <string>
#include <vector>

#include "imageio.h"
#include "renderer.h"
#include "sharded.h"
#include "vr_device.h"
#include "vr_math_probe.h"

struct vr_renderer {
    vr::RendererHIP impl;
    int device = 0;
};

// N renderers on N devices behind one frame (sharded.h).  The parts are ordinary vr_renderer objects owned by this object: every scene
// call of this header applies to them one by one (vr_sharded_part), which is how the scene is replicated.
struct vr_sharded {
    std::vector<vr_renderer*> parts;
    std::unique_ptr<vr::ShardedRenderer> impl;
    std::string transport, collective;
};

static thread_local std::string g_last_error;

static int guard(const std::function<void()>& fn) {
    try {
        fn();
        g_last_error.clear();
        return VR_OK;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return VR_ERR;
    } catch (...) {
        g_last_error = "unknown error";
        return VR_ERR;
    }
}
static int fail(int code, const char* msg) { g_last_error = msg; return code; }
#define NEED(r) do { if (!(r)) return fail(VR_ERR_ARG, "null renderer"); } while (0)
#define NEED_SHARDED(s) do { if (!(s)) return fail(VR_ERR_ARG, "null sharded renderer"); } while (0)
#define NEED_DEVICE() do { if (vr_device_count() <= 0) return fail(VR_ERR_NO_DEVICE, "no HIP device available (libvolren_amd has no CPU path)"); } while (0)

static void use_device(vr_renderer* r) { VR_HIP(hipSetDevice(r->device)); }

// A whole-frame read-back of the denoiser's data: the renderer, the output, then the device are checked before the renderer is touched.
static int read_back(vr_renderer* r, float* out, void (vr::RendererHIP::*download)(float*)) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    NEED_DEVICE();
    return guard([&] { use_device(r); (r->impl.*download)(out); });
}

namespace {
using Rn = vr::RendererHIP;
// The int parameters, one row each: the name, how it is read, how it is written (none: read-only), the accepted range (none where lo > hi) and what
// a value outside it is answered with.  vr_set_int and vr_get_int are lookups here.  A writer may refuse by itself: the ones that need more than a range.
struct IntParam {
    const char* name;
    int (*get)(Rn&);
    void (*set)(Rn&, int);
    int lo, hi;
    const char* refusal;
};
vr::SceneParams next_launch(Rn& R) { vr::SceneParams P; R.fill_params(P); return P; }      // the scene as the current frame's next launch will read it
vr::PathtraceKernel next_kernel(Rn& R) { return vr::pathtrace_kernel_of(next_launch(R), R.tuning.wide_addressing != 0, R.tuning.stats != nullptr); }      // ... and the kernel that serves it (vr_variant.h)
void set_grid_frame(Rn& R, int v) {
    if (!R.volume || v < 0 || (size_t)v >= R.volume->n_grid_frames()) throw std::runtime_error("grid_frame_counter out of range");
    R.volume->grid_frame_counter = (size_t)v;
}
#define VR_GET(expr) [](Rn& R) -> int { return expr; }
#define VR_SET(stmt) [](Rn& R, int v) { stmt; }
#define VR_INT(field) VR_GET(R.field), VR_SET(R.field = v)
#define VR_FLAG(field) VR_GET(R.field ? 1 : 0), VR_SET(R.field = v != 0)      // any value but 0 switches it on
#define VR_ANY 1, 0, nullptr
#define VR_READ_ONLY(expr) VR_GET(expr), nullptr, VR_ANY
const IntParam kIntParams[] = {
    { "sample", VR_GET(R.sample), VR_SET(R.sample = v; R.drop_tile_samples()), VR_ANY },      // a count set by hand is a uniform frame's (include/volren_amd.h: ragged frames)
    { "sppx", VR_INT(sppx), VR_ANY },
    { "seed", VR_INT(seed), VR_ANY },
    { "bounces", VR_INT(bounces), VR_ANY },
    { "show_environment", VR_FLAG(show_environment), VR_ANY },
    { "tonemapping", VR_FLAG(tonemapping), VR_ANY },
    { "integrator", VR_INT(integrator), VR_ANY },
    { "fast_math", VR_FLAG(fast_math), VR_ANY },
    { "variance", VR_INT(variance), 0, 1, "variance: 0 (off) or 1 (keep the per-pixel second moments)" },
    { "denoise_iterations", VR_INT(denoise_iterations), 0, vr::kDenoiseMaxIterations, "denoise_iterations must be in [0, 10]" },
    { "denoise_moments", VR_GET(R.denoise_moments), VR_SET(R.set_denoise_moments(v)), VR_ANY },
    { "denoise_resolve", VR_GET(R.denoise_resolve), VR_SET(R.set_denoise_resolve(v)), VR_ANY },
    { "denoise_layers", VR_GET(R.denoise_layers), VR_SET(R.set_denoise_layers(v)), VR_ANY },
    { "denoise_filter", VR_GET(R.denoise_filter), VR_SET(R.set_denoise_filter(v)), VR_ANY },
    { "denoise_demodulate", VR_GET(R.denoise_demodulate), VR_SET(R.set_denoise_demodulate(v)), VR_ANY },
    { "coalesce_trace", VR_GET(R.coalesce_trace ? 1 : 0), VR_SET(R.flush_pending(); R.coalesce_trace = v != 0), VR_ANY },
    { "majorant_layout", VR_INT(majorant_layout), -1, 1, "majorant_layout: -1 (per grid, chosen at commit), 0 (linear), 1 (4x4x4-cell blocks)" },
    { "majorant_blocked", VR_READ_ONLY(next_launch(R).density.maj_blocked) },
    // which compiled kernel the next launch uses, and what sent it to the run-time one (vr_variant.h PathtraceVariantReason)
    { "kernel_variant", VR_READ_ONLY(next_kernel(R).variant) },
    { "kernel_variant_reason", VR_READ_ONLY(next_kernel(R).reason) },
    { "tf_float_atlas", VR_FLAG(tf_float_atlas), VR_ANY },
    { "wide_addressing", VR_INT(tuning.wide_addressing), 0, 1, "wide_addressing: 0 (by the tables' sizes), 1 (always the kernels with 64-bit gather addresses)" },
    // the next launch's kernel forms 64-bit gather addresses: forced, a table of 4 GiB or more, or a variant that always does (2, 3, 4)
    { "kernel_wide", VR_READ_ONLY(next_kernel(R).wide ? 1 : 0) },
    { "env_div_safe", VR_READ_ONLY(R.environment && R.environment->cdf_div_safe ? 1 : 0) },      // the environment's warp table passed env_cdf_kernel's check (vr_math.h div_core)
    { "env_compact", VR_READ_ONLY(R.environment && R.environment->envmap_rgbe ? 1 : 0) },      // the path tracer fetches the map's texels as RGBE dwords (vr_scene.h SceneParams::env_rgbe)
    { "pending_samples", VR_READ_ONLY(R.pending_samples()) },
    { "gpu_encoder", VR_FLAG(gpu_encoder), VR_ANY },
    { "sample_pool_mb", VR_GET((int)(R.sample_pool_bytes >> 20)), VR_SET(R.sample_pool_bytes = (size_t)v << 20), 16, 65536,
      "sample_pool_mb must be in [16, 65536] (item indices of a sub-launch are 32-bit: < 2^32 RGBA32F items)" },
    { "seed_table_mb", VR_GET(R.seed_table_budget_mb()), VR_SET(R.seed_table_mb = v), -1, Rn::kSeedTableMaxMb,      // reads back the budget -1 resolves to
      "seed_table_mb must be in [0, 8192] (0 = no table), or -1 for the default min(4096, sample_pool_mb / 4)" },
    { "seed_table_max_samples", VR_INT(seed_table_max_samples), 0, INT_MAX, "seed_table_max_samples must be >= 0 (0 = as many as seed_table_mb holds)" },
    { "seed_table_samples", VR_READ_ONLY(R.seed_table_samples()) },
    { "seed_table_fills", VR_READ_ONLY(R.seed_table_fills()) },
    { "launch_target_ms", VR_INT(launch_target_ms), 0, INT_MAX, "launch_target_ms must be >= 0 (0 = no sizing by time)" },
    { "expected_skip", VR_INT(expected_skip), 0, 1, "expected_skip: 0 (march every step) or 1 (drop the steps of empty space by the clear-distance table)" },
    { "expected_field", VR_INT(expected_field), 0, 1, "expected_field: 0 (march the trilinear field) or 1 (the tracker's field: without a LUT the cubic B-spline field)" },
    { "expected_stats", VR_INT(expected_stats), 0, 1, "expected_stats: 0 (off) or 1 (the expected-value passes count their work)" },
    { "order_tiles", VR_INT(order_tiles), 0, 2, "order_tiles: 0 (never), 1 (tile subsets), 2 (always)" },
    { "sky_tiles", VR_INT(sky_tiles), 0, 1, "sky_tiles: 0 (every tile through the path tracer) or 1 (tiles whose camera rays cannot hit the volume's box are rendered apart)" },
    { "last_sky_tiles", VR_READ_ONLY(R.last_sky_tiles) },
    { "see_through_tiles", VR_INT(see_through_tiles), 0, 1, "see_through_tiles: 0 or 1 (where the clear tiles are rendered apart, so are the tiles whose camera rays cross the box without reaching a voxel with density)" },
    { "last_see_through_tiles", VR_READ_ONLY(R.last_see_through_tiles) },
    { "grid_frame_counter", VR_GET(R.volume ? (int)R.volume->grid_frame_counter : 0), set_grid_frame, VR_ANY },
    { "n_grid_frames", VR_READ_ONLY(R.volume ? (int)R.volume->n_grid_frames() : 0) },
    { "last_launches", VR_READ_ONLY(R.last_launches) },
    { "adaptive_rounds", VR_READ_ONLY(R.adaptive_rounds) },
    { "width", VR_READ_ONLY(R.resolution.x) },
    { "height", VR_READ_ONLY(R.resolution.y) },
};
#undef VR_GET
#undef VR_SET
#undef VR_INT
#undef VR_FLAG
#undef VR_ANY
#undef VR_READ_ONLY
// the row of `name`; `writable`: a read-only name is as unknown to vr_set_int as any other
const IntParam& int_param(const char* name, bool writable) {
    for (const IntParam& p : kIntParams)
        if (!strcmp(p.name, name) && (p.set || !writable)) return p;
    throw std::runtime_error(std::string("unknown int parameter: ") + name);
}

// The float parameters, one row each: where the values live, how many they are and, where they have a range, the check vr_set_float runs on the
// caller's values.  The check comes before the count is compared, so it sees the caller's count: denoise_sigma answers a wrong one in its own words.
struct FloatField { float* ptr; int count; void (*check)(const float* values, int count) = nullptr; };
FloatField float_field(vr::RendererHIP& R, const std::string& n) {
    if (n == "tonemap_exposure") return { &R.tonemap_exposure, 1 };
    if (n == "tonemap_gamma") return { &R.tonemap_gamma, 1 };
    if (n == "albedo") return { &R.albedo.x, 3 };
    if (n == "phase") return { &R.phase, 1 };
    if (n == "density_scale") return { &R.density_scale, 1 };
    if (n == "emission_scale") return { &R.emission_scale, 1 };
    if (n == "vol_clip_min") return { &R.vol_clip_min.x, 3 };
    if (n == "vol_clip_max") return { &R.vol_clip_max.x, 3 };
    if (n == "cam_pos") return { &R.camera.pos.x, 3 };
    if (n == "cam_dir") return { &R.camera.dir.x, 3 };
    if (n == "cam_up") return { &R.camera.up.x, 3 };
    if (n == "cam_fov") return { &R.camera.fov_degree, 1 };
    if (n == "env_strength") { if (!R.environment) throw std::runtime_error("no environment"); return { &R.environment->strength, 1 }; }
    if (n == "env_transform") { if (!R.environment) throw std::runtime_error("no environment"); return { R.environment->transform.m, 9 }; }
    if (n == "tf_window_left") { if (!R.transferfunc) throw std::runtime_error("no transfer function"); return { &R.transferfunc->window_left, 1 }; }
    if (n == "tf_window_width") { if (!R.transferfunc) throw std::runtime_error("no transfer function"); return { &R.transferfunc->window_width, 1 }; }
    if (n == "volume_transform") { if (!R.volume) throw std::runtime_error("no volume"); return { R.volume->transform.m, 16 }; }
    if (n == "denoise_sigma") return { R.denoise_sigma, 5, [](const float* values, int count) {      // colour, normal, depth, coverage, albedo: each in [2^-60, 2^60] (vr_denoise.h)
        if (count != 5) throw std::runtime_error("denoise_sigma takes 5 values (colour, normal, depth, coverage, albedo)");
        for (int i = 0; i < 5; ++i)
            if (!(values[i] >= vr::kDenoiseSigmaMin && values[i] <= vr::kDenoiseSigmaMax))
                throw std::runtime_error("denoise_sigma: every value must be in [2^-60, 2^60]");
    } };
    if (n == "denoise_alpha") return { &R.denoise_alpha, 1, [](const float* values, int count) {      // vr_temporal.h
        if (count == 1 && !(values[0] >= vr::kTemporalAlphaMin && values[0] <= vr::kTemporalAlphaMax)) throw std::runtime_error("denoise_alpha must be in [2^-20, 1]");
    } };
    if (n == "denoise_reject") return { &R.denoise_reject, 1, [](const float* values, int count) {
        if (count == 1 && !(values[0] == 0.0f || (values[0] >= vr::kTemporalRejectMin && values[0] <= vr::kTemporalRejectMax)))
            throw std::runtime_error("denoise_reject must be 0 (off) or in [2^-10, 2^20]");
    } };
    if (n == "denoise_ridge") return { &R.denoise_ridge, 1, [](const float* values, int count) {      // vr_regress.h
        if (count == 1 && !vr::regress_ridge_ok(values[0])) throw std::runtime_error("denoise_ridge must be 0 (zero order) or in [2^-20, 2^20]");
    } };
    throw std::runtime_error("unknown float parameter: " + n);
}
}  // namespace

extern "C" {

const char* vr_last_error(void) { return g_last_error.c_str(); }
const char* vr_version(void) { return "volren_amd 0.1 (gfx950)"; }

int vr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vr_create(vr_renderer** out, int device, int width, int height) {
    if (!out) return fail(VR_ERR_ARG, "null out pointer");
    *out = nullptr;
    NEED_DEVICE();
    vr_renderer* r = nullptr;
    const int rc = guard([&] {
        if (width <= 0 || height <= 0) throw std::runtime_error("vr_create: resolution must be positive");
        r = new vr_renderer();
        r->device = device;
        use_device(r);
        r->impl.resolution = { width, height };
        r->impl.init();
    });
    if (rc != VR_OK) { delete r; return rc; }
    *out = r;
    return VR_OK;
}

void vr_destroy(vr_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;
}

int vr_resize(vr_renderer* r, int w, int h) {
    NEED(r);
    return guard([&] { use_device(r); if (w <= 0 || h <= 0) throw std::runtime_error("vr_resize: resolution must be positive"); r->impl.resize((uint32_t)w, (uint32_t)h); r->impl.sample = 0; });
}

// main.cpp:37-62
int vr_load_volume(vr_renderer* r, const char* path) {
    NEED(r);
    if (!path) return fail(VR_ERR_ARG, "null path");
    return guard([&] {
        use_device(r);
        std::cout << "load volume: " << path << std::endl;
        if (std::filesystem::is_directory(path)) r->impl.volume = vr::Volume::load_folder(path);
        else r->impl.volume = std::make_shared<vr::Volume>(std::string(path));
        r->impl.density_scale = 1.f;
        r->impl.scale_and_move_to_unit_cube();
        r->impl.commit();
        r->impl.sample = 0;
    });
}

// renderer.volume = std::make_shared<voldata::Volume>(path) as the Python scripts do it (bindings.cpp:82,176;
// datagen_colmap.py:57, datagen_denoise.py:85): ONLY replaces the volume -- density_scale, the unit-cube transform and the
// device grids are untouched until the caller runs scale_and_move_to_unit_cube() / commit() itself
int vr_set_volume_path(vr_renderer* r, const char* path) {
    NEED(r);
    if (!path) return fail(VR_ERR_ARG, "null path");
    return guard([&] {
        if (std::filesystem::is_directory(path)) r->impl.volume = vr::Volume::load_folder(path);
        else r->impl.volume = std::make_shared<vr::Volume>(std::string(path));
    });
}

// voldata::Volume::AABB(name) / minorant_majorant(name) of the renderer's volume (bindings.cpp:91,93): world-space box of the
// current frame's grid under the volume transform, out = min xyz, max xyz
int vr_volume_aabb(vr_renderer* r, const char* name, float out[6]) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null output");
    return guard([&] {
        if (!r->impl.volume || r->impl.volume->grids.empty()) throw std::runtime_error("vr_volume_aabb: no volume");
        const auto bb = r->impl.volume->AABB(name ? name : "density");
        out[0] = bb.first.x; out[1] = bb.first.y; out[2] = bb.first.z; out[3] = bb.second.x; out[4] = bb.second.y; out[5] = bb.second.z;
    });
}
int vr_volume_minorant_majorant(vr_renderer* r, const char* name, float out[2]) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null output");
    return guard([&] {
        if (!r->impl.volume || r->impl.volume->grids.empty()) throw std::runtime_error("vr_volume_minorant_majorant: no volume");
        const auto mm = r->impl.volume->minorant_majorant(name ? name : "density");
        out[0] = mm.first; out[1] = mm.second;
    });
}

// main.cpp:64-71
int vr_load_envmap(vr_renderer* r, const char* path) {
    NEED(r);
    if (!path) return fail(VR_ERR_ARG, "null path");
    return guard([&] { use_device(r); r->impl.environment = std::make_shared<vr::Environment>(std::string(path)); r->impl.sample = 0; });
}

// main.cpp:73-81
int vr_load_transferfunc(vr_renderer* r, const char* path) {
    NEED(r);
    if (!path) return fail(VR_ERR_ARG, "null path");
    return guard([&] {
        use_device(r);
        r->impl.transferfunc = std::make_shared<vr::TransferFunction>(std::string(path));
        r->impl.show_environment = false;
        r->impl.sample = 0;
    });
}

static void install_grid(vr_renderer* r, const char* name, const std::shared_ptr<vr::Grid>& grid, int unit_cube) {
    const std::string n = name ? name : "density";
    auto& R = r->impl;
    if (n == "density") {
        R.volume = std::make_shared<vr::Volume>(grid);
        if (unit_cube) { R.density_scale = 1.f; R.scale_and_move_to_unit_cube(); }
    } else {
        if (!R.volume || R.volume->grids.empty()) throw std::runtime_error("set the density grid before '" + n + "'");
        R.volume->update_grid_frame(R.volume->grid_frame_counter, grid, n);
    }
    R.sample = 0;
}

int vr_set_volume_dense(vr_renderer* r, const char* name, const float* voxels, int nx, int ny, int nz, const float* transform, int unit_cube) {
    NEED(r);
    if (!voxels || nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_ARG, "bad dense grid arguments");
    return guard([&] {
        use_device(r);
        auto g = std::make_shared<vr::DenseGrid>((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, voxels);
        if (transform) memcpy(g->transform.m, transform, 64);
        install_grid(r, name, g, unit_cube);
    });
}

// voldata::Volume::add_grid_frame / update_grid_frame (src/bindings.cpp:89-90) for dense float grids: a further animation frame holding
// `name`, or grid `name` of frame `frame` replaced.  Takes effect at the next vr_commit(), like every change of the volume.
int vr_volume_add_grid_frame_dense(vr_renderer* r, const char* name, const float* voxels, int nx, int ny, int nz, const float* transform) {
    NEED(r);
    if (!voxels || nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_ARG, "bad dense grid arguments");
    return guard([&] {
        auto g = std::make_shared<vr::DenseGrid>((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, voxels);
        if (transform) memcpy(g->transform.m, transform, 64);
        if (!r->impl.volume) r->impl.volume = std::make_shared<vr::Volume>();
        r->impl.volume->add_grid_frame(g, name ? name : "density");
        r->impl.sample = 0;
    });
}
int vr_volume_update_grid_frame_dense(vr_renderer* r, int frame, const char* name, const float* voxels, int nx, int ny, int nz, const float* transform) {
    NEED(r);
    if (!voxels || nx <= 0 || ny <= 0 || nz <= 0 || frame < 0) return fail(VR_ERR_ARG, "bad dense grid arguments");
    return guard([&] {
        if (!r->impl.volume || (size_t)frame >= r->impl.volume->n_grid_frames()) throw std::out_of_range("vr_volume_update_grid_frame_dense: no such frame");
        auto g = std::make_shared<vr::DenseGrid>((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, voxels);
        if (transform) memcpy(g->transform.m, transform, 64);
        r->impl.volume->update_grid_frame((size_t)frame, g, name ? name : "density");
        r->impl.sample = 0;
    });
}
int vr_volume_n_grid_frames(vr_renderer* r, int* n) {
    NEED(r);
    if (!n) return fail(VR_ERR_ARG, "null output");
    *n = r->impl.volume ? (int)r->impl.volume->n_grid_frames() : 0;
    return VR_OK;
}

int vr_set_volume_dense_f16(vr_renderer* r, const char* name, const uint16_t* voxels, int nx, int ny, int nz, const float* transform, int unit_cube) {
    NEED(r);
    if (!voxels || nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_ARG, "bad dense grid arguments");
    return guard([&] {
        use_device(r);
        auto g = std::make_shared<vr::DenseGridF16>((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, voxels);
        if (transform) memcpy(g->transform.m, transform, 64);
        install_grid(r, name, g, unit_cube);
    });
}

int vr_set_volume_brick(vr_renderer* r, const char* name, const float* transform, const uint32_t nb[3], const float min_maj[2],
                        const uint32_t* indirection, const uint32_t* range, const uint32_t atlas_dim[3], const uint8_t* atlas,
                        int n_mips, const uint32_t* const* mips, const uint32_t (*mip_dims)[3], int unit_cube) {
    NEED(r);
    if (!nb || !min_maj || !indirection || !range || !atlas_dim || !atlas || n_mips < 0 || n_mips > 3) return fail(VR_ERR_ARG, "bad brick grid arguments");
    return guard([&] {
        use_device(r);
        auto g = std::make_shared<vr::BrickGrid>();
        if (transform) memcpy(g->transform.m, transform, 64);
        g->n_bricks = { nb[0], nb[1], nb[2] };
        g->min_maj = { min_maj[0], min_maj[1] };
        const size_t n = (size_t)nb[0] * nb[1] * nb[2];
        g->indirection = vr::Buf3D<uint32_t>(nb[0], nb[1], nb[2]);
        g->range = vr::Buf3D<uint32_t>(nb[0], nb[1], nb[2]);
        memcpy(g->indirection.data.data(), indirection, n * 4);
        memcpy(g->range.data.data(), range, n * 4);
        if ((atlas_dim[0] % 8) || (atlas_dim[1] % 8) || (atlas_dim[2] % 8)) throw std::runtime_error("atlas dimensions must be multiples of 8");
        g->atlas = vr::Buf3D<uint8_t>(atlas_dim[0], atlas_dim[1], atlas_dim[2]);
        memcpy(g->atlas.data.data(), atlas, g->atlas.data.size());
        uint64_t cnt = 0;
        for (size_t i = 0; i < n; ++i) cnt += (vr::half2float(range[i] & 0xFFFFu) != vr::half2float(range[i] >> 16));
        g->brick_counter = cnt;
        for (int m = 0; m < n_mips; ++m) {
            vr::Buf3D<uint32_t> b(mip_dims[m][0], mip_dims[m][1], mip_dims[m][2]);
            memcpy(b.data.data(), mips[m], b.data.size() * 4);
            g->range_mipmaps.push_back(std::move(b));
        }
        install_grid(r, name, g, unit_cube);
    });
}

int vr_set_envmap(vr_renderer* r, const float* rgb, int w, int h) {
    NEED(r);
    if (!rgb || w <= 0 || h <= 0) return fail(VR_ERR_ARG, "bad envmap arguments");
    return guard([&] { use_device(r); r->impl.environment = std::make_shared<vr::Environment>(rgb, w, h); r->impl.sample = 0; });
}

int vr_set_transferfunc(vr_renderer* r, const float* rgba, int n) {
    NEED(r);
    return guard([&] {
        use_device(r);
        if (n <= 0 || !rgba) { r->impl.transferfunc.reset(); r->impl.sample = 0; return; }
        std::vector<vr::vec4> lut;
        for (int i = 0; i < n; ++i) lut.emplace_back(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3]);
        r->impl.transferfunc = std::make_shared<vr::TransferFunction>(lut);
        r->impl.sample = 0;
    });
}

int vr_set_int(vr_renderer* r, const char* name, int v) {
    NEED(r);
    if (!name) return fail(VR_ERR_ARG, "null name");
    return guard([&] {
        const IntParam& p = int_param(name, true);
        if (p.lo <= p.hi && (v < p.lo || v > p.hi)) throw std::runtime_error(p.refusal);
        p.set(r->impl, v);
    });
}

int vr_get_int(vr_renderer* r, const char* name, int* v) {
    NEED(r);
    if (!name || !v) return fail(VR_ERR_ARG, "null argument");
    return guard([&] { *v = int_param(name, false).get(r->impl); });
}

int vr_set_float(vr_renderer* r, const char* name, const float* values, int count) {
    NEED(r);
    if (!name || !values) return fail(VR_ERR_ARG, "null argument");
    return guard([&] {
        auto& R = r->impl;
        const std::string n = name;
        if (n == "env_rot") {                       // main.cpp:381-382
            if (count != 1) throw std::runtime_error("env_rot takes 1 value");
            if (!R.environment) throw std::runtime_error("no environment");
            R.environment->transform = vr::rotation_axis(values[0], 1);
            return;
        }
        if (n == "albedo" && count == 1) { R.albedo = vr::vec3(values[0]); return; }      // main.cpp:371-372
        const FloatField f = float_field(R, n);
        if (f.check) f.check(values, count);
        if (count != f.count) throw std::runtime_error("wrong value count for " + n);
        memcpy(f.ptr, values, sizeof(float) * (size_t)count);
    });
}

int vr_get_float(vr_renderer* r, const char* name, float* values, int count) {
    NEED(r);
    if (!name || !values) return fail(VR_ERR_ARG, "null argument");
    return guard([&] {
        const FloatField f = float_field(r->impl, name);
        if (count != f.count) throw std::runtime_error(std::string("wrong value count for ") + name);
        memcpy(values, f.ptr, sizeof(float) * (size_t)count);
    });
}

int vr_commit(vr_renderer* r) { NEED(r); return guard([&] { use_device(r); r->impl.commit(); }); }
int vr_reset(vr_renderer* r) { NEED(r); return guard([&] { r->impl.reset(); }); }
int vr_scale_and_move_to_unit_cube(vr_renderer* r) { NEED(r); return guard([&] { r->impl.scale_and_move_to_unit_cube(); }); }

int vr_trace(vr_renderer* r) { NEED(r); return guard([&] { use_device(r); r->impl.trace(); }); }
int vr_flush(vr_renderer* r) { NEED(r); return guard([&] { use_device(r); r->impl.flush_pending(); }); }
int vr_render(vr_renderer* r, int spp) { NEED(r); return guard([&] { use_device(r); r->impl.render(spp); }); }

int vr_synchronize(vr_renderer* r) {
    NEED(r);
    return guard([&] {
        use_device(r);
        r->impl.synchronize();
        r->impl.check_watchdog();
    });
}

int vr_last_kernel_ms(vr_renderer* r, double* ms) {
    NEED(r);
    if (!ms) return fail(VR_ERR_ARG, "null argument");
    return guard([&] { use_device(r); *ms = r->impl.last_kernel_ms(); });
}

int vr_last_pathtrace_ms(vr_renderer* r, double* ms) {
    NEED(r);
    if (!ms) return fail(VR_ERR_ARG, "null output");
    return guard([&] { use_device(r); *ms = r->impl.last_pathtrace_ms(); });
}

int vr_framebuffer(vr_renderer* r, float* out) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    return guard([&] { use_device(r); r->impl.download(out); });
}
// denoiser data: the device is checked before the renderer is touched
int vr_render_features(vr_renderer* r, int spp) {
    NEED(r);
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.render_features(spp); });
}
int vr_render_features_expected(vr_renderer* r, int rays) {
    NEED(r);
    if (rays < 1 || rays > vr::kExpectedMaxRays) return fail(VR_ERR_ARG, "vr_render_features_expected: rays must be 1..4");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.render_features_expected(rays); });
}
int vr_expected_stats(vr_renderer* r, uint64_t out[4]) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.expected_stats_read(out); });
}
int vr_expected_clear_table(vr_renderer* r, uint8_t* out, int cells[3]) {
    NEED(r);
    if (!cells) return fail(VR_ERR_ARG, "null argument");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.expected_clear_table(out, cells); });
}
int vr_features(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_features); }
int vr_variance(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_variance); }
int vr_denoise(vr_renderer* r) {
    NEED(r);
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.denoise(); });
}
int vr_denoise_temporal(vr_renderer* r) {
    NEED(r);
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.denoise_temporal(); });
}
int vr_denoise_history_reset(vr_renderer* r) {
    NEED(r);
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.flush_pending(); r->impl.drop_history(); });
}
int vr_denoise_history(vr_renderer* r, float* rgba_out, float* var_out, float* length_out) {
    NEED(r);
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.download_history(rgba_out, var_out, length_out); });
}
int vr_denoise_reject_stat(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_reject_stat); }
int vr_denoise_history_moments(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_history_moments); }
// (the refusals read host state only: they come before the device is asked for)
int vr_resolve(vr_renderer* r) {
    NEED(r);
    if (const int rc = guard([&] { r->impl.check_resolve("resolve: ", false); })) return rc;
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.resolve(); });
}
int vr_resolved(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_resolved); }
int vr_resolve_background(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_resolve_background); }
int vr_denoised_layer(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_denoised_layer); }
int vr_upsample(vr_renderer* r, int factor, int rays) {
    NEED(r);
    if (factor < 2 || factor > 4) return fail(VR_ERR_ARG, "vr_upsample: factor must be 2..4");
    if (rays < 1 || rays > vr::kExpectedMaxRays) return fail(VR_ERR_ARG, "vr_upsample: rays must be 1..4");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.upsample(factor, rays); });
}
int vr_upsampled(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_upsampled); }
int vr_upsampled_layer(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_upsampled_layer); }
int vr_upsampled_features(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_upsampled_features); }
int vr_upsampled_size(vr_renderer* r, int wh[2]) {
    NEED(r);
    if (!wh) return fail(VR_ERR_ARG, "null argument");
    NEED_DEVICE();
    return guard([&] { r->impl.upsampled_size(wh); });
}
int vr_denoised(vr_renderer* r, float* out) { return read_back(r, out, &vr::RendererHIP::download_denoised); }
// adaptive sampling: the arguments, then the device, are checked before the renderer is touched
int vr_render_adaptive(vr_renderer* r, int min_spp, int max_spp, float threshold) {
    NEED(r);
    if (min_spp < 2 || min_spp > max_spp || !(threshold >= 0.0f) || !std::isfinite(threshold))
        return fail(VR_ERR_ARG, "vr_render_adaptive: needs 2 <= min_spp <= max_spp and a finite threshold >= 0");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.render_adaptive(min_spp, max_spp, threshold); });
}
static int tile_count_arg(vr_renderer* r, int n_tiles) {
    const auto& res = r->impl.resolution;
    return n_tiles == vr::tile_count(res.x, res.y) ? VR_OK : fail(VR_ERR_ARG, "n_tiles must be ceil(W / 16) * ceil(H / 16)");
}
int vr_tile_samples(vr_renderer* r, int32_t* out, int n_tiles) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    NEED_DEVICE();
    if (tile_count_arg(r, n_tiles) != VR_OK) return VR_ERR_ARG;
    return guard([&] {
        use_device(r);
        r->impl.synchronize();
        const std::vector<int32_t> c = r->impl.tile_samples();
        std::copy(c.begin(), c.end(), out);
    });
}
int vr_tile_error(vr_renderer* r, float* out, int n_tiles) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    NEED_DEVICE();
    if (tile_count_arg(r, n_tiles) != VR_OK) return VR_ERR_ARG;
    return guard([&] {
        use_device(r);
        const std::vector<float> e = r->impl.tile_error();
        std::copy(e.begin(), e.end(), out);
    });
}
int vr_framebuffer_device(vr_renderer* r, void** p) {
    NEED(r);
    if (!p) return fail(VR_ERR_ARG, "null argument");
    return guard([&] { if (!r->impl.color) throw std::runtime_error("no framebuffer"); use_device(r); r->impl.flush_pending(); *p = r->impl.color->get(); });
}
int vr_draw(vr_renderer* r) { NEED(r); return guard([&] { use_device(r); r->impl.draw(); }); }
int vr_display(vr_renderer* r, float* out) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    return guard([&] { use_device(r); r->impl.download_display(out); });
}
int vr_save_png(vr_renderer* r, const char* path) {
    NEED(r);
    if (!path) return fail(VR_ERR_ARG, "null path");
    return guard([&] {
        use_device(r);
        auto& R = r->impl;
        R.draw();
        std::vector<float> fb((size_t)R.resolution.x * R.resolution.y * 4);
        R.download_display(fb.data());
        std::vector<uint8_t> rgba;
        vr::framebuffer_to_rgba8(fb.data(), R.resolution.x, R.resolution.y, rgba);
        vr::save_png_rgba8(path, rgba.data(), R.resolution.x, R.resolution.y);
    });
}

int vr_set_tiles(vr_renderer* r, const int32_t* ids, int n) {
    NEED(r);
    return guard([&] {
        use_device(r);
        std::vector<int32_t> t;
        if (n > 0 && ids) t.assign(ids, ids + n);
        r->impl.set_tiles(t);
    });
}
int vr_set_stream(vr_renderer* r, void* s) { NEED(r); return guard([&] { use_device(r); r->impl.flush_pending(); r->impl.stream = (hipStream_t)s; }); }

int vr_pack_tiles(vr_renderer* r, const int32_t* ids_dev, int n, void* packed) {
    NEED(r);
    return guard([&] {
        use_device(r);
        auto& R = r->impl;
        if (!R.color) throw std::runtime_error("no framebuffer");
        R.flush_pending();
        vr::launch_pack_tiles(R.color->as<float>(), R.resolution.x, R.resolution.y, ids_dev, n, (float*)packed, R.stream);
        VR_HIP(hipGetLastError());
    });
}
int vr_unpack_tiles(vr_renderer* r, const int32_t* ids_dev, int n, const void* packed) {
    NEED(r);
    return guard([&] {
        use_device(r);
        auto& R = r->impl;
        if (!R.color) throw std::runtime_error("no framebuffer");
        R.flush_pending();
        vr::launch_unpack_tiles((const float*)packed, ids_dev, n, R.color->as<float>(), R.resolution.x, R.resolution.y, R.stream);
        VR_HIP(hipGetLastError());
    });
}

int vr_grid_checksums(vr_renderer* r, uint64_t out[3]) {
    NEED(r);
    if (!out) return fail(VR_ERR_ARG, "null argument");
    return guard([&] {
        use_device(r);
        auto& R = r->impl;
        if (!R.volume || R.density_grids.empty()) throw std::runtime_error("no committed volume");
        R.grid_checksums(R.density_grids.at(R.volume->grid_frame_counter), out);
    });
}

// ---- one frame on several devices (sharded.h) ------------------------------------------------------------------------------
int vr_sharded_create(vr_sharded** out, const int* devices, int n_parts, int width, int height) {
    if (!out) return fail(VR_ERR_ARG, "null out pointer");
    *out = nullptr;
    if (!devices || n_parts <= 0 || n_parts > 64) return fail(VR_ERR_ARG, "vr_sharded_create: 1..64 parts, one device ordinal each");
    NEED_DEVICE();
    vr_sharded* s = new vr_sharded();
    const int rc = guard([&] {
        std::vector<vr::RendererHIP*> impls;
        std::vector<int> devs(devices, devices + n_parts);
        for (int i = 0; i < n_parts; ++i) {
            vr_renderer* r = nullptr;
            if (vr_create(&r, devices[i], width, height) != VR_OK) throw std::runtime_error(g_last_error);
            s->parts.push_back(r);
            impls.push_back(&r->impl);
        }
        s->impl = std::make_unique<vr::ShardedRenderer>(impls, devs);
        s->transport = s->impl->transport();
        s->collective = s->impl->collective();
    });
    if (rc != VR_OK) { const std::string keep = g_last_error; vr_sharded_destroy(s); g_last_error = keep; return rc; }
    *out = s;
    return VR_OK;
}
void vr_sharded_destroy(vr_sharded* s) {
    if (!s) return;
    s->impl.reset();                                  // waits for the parts' streams, gives them their default stream back
    for (vr_renderer* r : s->parts) vr_destroy(r);
    delete s;
}
int vr_sharded_parts(vr_sharded* s) { return s ? (int)s->parts.size() : 0; }
vr_renderer* vr_sharded_part(vr_sharded* s, int i) { return (s && i >= 0 && i < (int)s->parts.size()) ? s->parts[(size_t)i] : nullptr; }
const char* vr_sharded_transport(vr_sharded* s) { return s ? s->transport.c_str() : ""; }
const char* vr_sharded_collective(vr_sharded* s) { return s ? s->collective.c_str() : ""; }
int vr_sharded_reset(vr_sharded* s) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->reset(); });
}
int vr_sharded_render(vr_sharded* s, int spp) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->render(spp); });
}
int vr_sharded_render_features(vr_sharded* s, int spp) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->render_features(spp); });
}
int vr_sharded_render_features_expected(vr_sharded* s, int rays) {
    NEED_SHARDED(s);
    if (rays < 1 || rays > vr::kExpectedMaxRays) return fail(VR_ERR_ARG, "vr_sharded_render_features_expected: rays must be 1..4");
    return guard([&] { s->impl->render_features_expected(rays); });
}
int vr_sharded_gather_guides(vr_sharded* s) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->gather_guides(); });
}
int vr_sharded_denoise(vr_sharded* s) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->denoise(); });
}
int vr_sharded_denoise_temporal(vr_sharded* s) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->denoise_temporal(); });
}
int vr_sharded_synchronize(vr_sharded* s) {
    NEED_SHARDED(s);
    return guard([&] { s->impl->synchronize(); });
}

int vr_tile_owners(int width, int height, int n_parts, int32_t* owner_out, int n_tiles) {
    if (!owner_out || width <= 0 || height <= 0 || n_parts <= 0) return fail(VR_ERR_ARG, "vr_tile_owners: bad arguments");
    if (n_tiles != vr::tile_count(width, height)) return fail(VR_ERR_ARG, "vr_tile_owners: n_tiles must be ceil(width / 16) * ceil(height / 16)");
    return guard([&] {
        const auto lists = vr::tile_owner_lists(width, height, n_parts);
        for (size_t p = 0; p < lists.size(); ++p)
            for (int32_t t : lists[p]) owner_out[t] = (int32_t)p;
    });
}

// seed table (renderer.h): the default budget for a sample pool of `sample_pool_mb`, and the sample numbers a budget of `mb` covers on a frame (host only)
int vr_seed_table_default_mb(int sample_pool_mb) { return sample_pool_mb < 0 ? 0 : vr::RendererHIP::seed_table_default_mb(sample_pool_mb); }
int vr_seed_table_samples_for(int mb, int width, int height) { return vr::RendererHIP::seed_table_samples_for(mb, width, height); }

int vr_uniforms_size(void) { return (int)sizeof(vr::Uniforms); }
int vr_get_uniforms(vr_renderer* r, void* out, int bytes) {
    NEED(r);
    if (!out || bytes != (int)sizeof(vr::Uniforms)) return fail(VR_ERR_ARG, "bad uniforms buffer");
    return guard([&] { use_device(r); vr::SceneParams P; r->impl.fill_params(P); memcpy(out, &P.u, sizeof(vr::Uniforms)); });
}

int vr_impmap_floats(vr_renderer* r) {
    if (!r || !r->impl.environment) return 0;
    return (int)(r->impl.environment->impmap->size_bytes() / sizeof(float));
}
int vr_get_impmap(vr_renderer* r, float* out, int count) {
    NEED(r);
    if (!out || count != vr_impmap_floats(r)) return fail(VR_ERR_ARG, "bad impmap buffer");
    return guard([&] { use_device(r); const auto v = r->impl.environment->download_impmap(); memcpy(out, v.data(), v.size() * sizeof(float)); });
}

int vr_set_sched(vr_renderer* r, const int32_t thr[8]) {
    NEED(r);
    if (!thr) return fail(VR_ERR_ARG, "null argument");
    // the kernel packs each threshold into a byte: a batch size is a number of lanes (NEW / MARCH = low-water mark / COLLIDE / NEE / POSTNEE / ESCAPE:
    // 0..64, 0 = the default of COLLIDE), [1] caps the slots of a wavefront's pool (0 = all, else 1..192).  A NEW threshold above the pool size
    // would never trigger a batch and end in the watchdog: refused here instead.
    for (int i = 0; i < 8; ++i) {
        const int hi = i == 1 ? 192 : 64;
        if (thr[i] < 0 || thr[i] > hi) return fail(VR_ERR_ARG, i == 1 ? "vr_set_sched: the slot cap [1] must be in 0..192" : "vr_set_sched: batch thresholds must be in 0..64");
    }
    if (thr[1] > 0 && thr[0] > thr[1]) return fail(VR_ERR_ARG, "vr_set_sched: the NEW threshold [0] exceeds the slot cap [1]");
    for (int i = 0; i < 8; ++i) r->impl.tuning.thr[i] = thr[i];
    g_last_error.clear();
    return VR_OK;
}

// scheduler statistics of this renderer's path-tracing launches: enable != 0 zeroes its 32 device counters and switches its launches to the
// instrumented kernels; out (32 x u64, may be NULL) receives what was counted so far (layout: include/volren_amd.h)
int vr_sched_stats(vr_renderer* r, int enable, unsigned long long* out) {
    NEED(r);
    return guard([&] { use_device(r); r->impl.sched_stats(enable != 0, out); });
}

// diagnostics: (begin, queue empty, end) of every wavefront of the last instrumented launch, 100 MHz ticks; n_words = 3 x wavefronts wanted (<= 3 x 8192)
int vr_wave_timeline(vr_renderer* r, unsigned long long* out, int n_words) {
    NEED(r);
    if (!out || n_words <= 0) return fail(VR_ERR_ARG, "bad arguments");
    return guard([&] { use_device(r); r->impl.wave_timeline(out, (size_t)n_words); });
}

// test hook (devmem.h): device allocations above `mb` MiB fail as if the device were out of memory; mb < 0 removes the cap
int vr_test_alloc_cap_mb(long long mb) {
    vr::test_alloc_cap().store(mb < 0 ? ~(size_t)0 : (size_t)mb << 20);
    return VR_OK;
}

int vr_math_probe(int fn, const float* a, const float* b, float* out, int n) {
    if (!a || !b || !out || n <= 0) return fail(VR_ERR_ARG, "bad arguments");
    if (vr_device_count() <= 0) return fail(VR_ERR_NO_DEVICE, "no HIP device available");
    return guard([&] {
        vr::DeviceBuffer da((size_t)n * 4), db((size_t)n * 4), dout((size_t)n * 4);
        da.upload(a, (size_t)n * 4); db.upload(b, (size_t)n * 4);
        vr::launch_math_probe(fn, da.as<float>(), db.as<float>(), dout.as<float>(), n, nullptr);
        VR_HIP(hipGetLastError());
        dout.download(out, (size_t)n * 4);
    });
}

// bit-pattern sweep: out[i] = f(bits(first + i), b) for i < count, one launch; fn >= 100: the tolerance-mode form fn - 100 (vr_fastprobe.hip)
int vr_math_sweep(int fn, uint32_t first, long long count, float b, float* out) {
    if (!out || count <= 0) return fail(VR_ERR_ARG, "bad arguments");
    if (count > (1ll << 26)) return fail(VR_ERR_ARG, "vr_math_sweep: at most 2^26 bit patterns per call");
    if (fn < 0 || fn == 17 || (fn >= vr::kMathProbeCodes && (fn < 100 || fn > 103))) return fail(VR_ERR_ARG, "vr_math_sweep: no such function code");
    if (vr_device_count() <= 0) return fail(VR_ERR_NO_DEVICE, "no HIP device available");
    return guard([&] {
        vr::DeviceBuffer dout((size_t)count * 4);
        if (fn >= 100) vr::launch_fast_math_sweep(fn - 100, first, dout.as<float>(), (int32_t)count, nullptr);
        else vr::launch_math_sweep(fn, first, b, dout.as<float>(), (int32_t)count, nullptr);
        VR_HIP(hipGetLastError());
        dout.download(out, (size_t)count * 4);
    });
}

int vr_probe(vr_renderer* r, int what, int form, const void* in, float* out, long long n) {
    NEED(r);
    if (!in || !out || n < 0) return fail(VR_ERR_ARG, "bad arguments");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.probe(what, form, static_cast<const uint32_t*>(in), out, (size_t)n); });
}

int vr_path_probe(vr_renderer* r, int kind, int form, const void* in, void* out, long long n) {
    NEED(r);
    if (!in || !out || n < 0) return fail(VR_ERR_ARG, "bad arguments");
    NEED_DEVICE();
    return guard([&] { use_device(r); r->impl.path_probe(kind, form, static_cast<const uint32_t*>(in), static_cast<uint32_t*>(out), (size_t)n); });
}

// test hook: one launcher of the image-space kernels on host arrays (include/volren_amd.h).  What needs no device is checked first; nullptr = the arguments are fine
static const char* filter_probe_error(int stage, int W, int H, const void* const* in, float* const* out, const float* p) {
    if (stage < 0 || stage > 8) return "vr_filter_probe: unknown stage";
    if (W < 1 || H < 1 || W > 4096 || H > 4096) return "vr_filter_probe: W and H must be in 1..4096";
    if (!in || !out || !p) return "vr_filter_probe: null argument";
    static const int need_in[9] = { 2, 3, 3, 2, 3, 3, 2, 3, 4 }, need_out[9] = { 2, 1, 3, 3, 1, 2, 1, 2, 1 };      // the arrays a stage cannot do without: the first of each list
    for (int k = 0; k < need_in[stage]; ++k) if (!in[k]) return "vr_filter_probe: a required input array is null";
    for (int k = 0; k < need_out[stage]; ++k) if (!out[k]) return "vr_filter_probe: a required output array is null";
    for (int k = 0; k < VR_FILTER_PROBE_PARAMS; ++k) if (!std::isfinite(p[k])) return "vr_filter_probe: a parameter is not finite";
    const float i0 = p[5], i1 = p[8];
    if (i0 != std::floor(i0) || i1 != std::floor(i1)) return "vr_filter_probe: an integer parameter is not whole";
    if (p[35] != 0.0f && p[35] != 1.0f) return "vr_filter_probe: demod must be 0 or 1";
    if (p[35] != 0.0f && stage != 0 && stage != 4 && stage != 5 && stage != 7) return "vr_filter_probe: demod = 1 goes with prepare, split, merge and upsample only";
    switch (stage) {
    case 0: if (i0 < 1.0f || i0 > 0x1p30f) return "vr_filter_probe: prepare needs 1 <= n <= 2^30"; break;
    case 1: if (i0 < 1.0f || i0 > 0x1p20f) return "vr_filter_probe: atrous needs 1 <= step <= 2^20"; break;
    case 2: {
        const bool have = in[3] != nullptr, moments = out[3] != nullptr;
        if (p[7] < 0.0f) return "vr_filter_probe: tau must be >= 0";
        if (moments && p[7] > 0.0f) return "vr_filter_probe: the moments form and the rejection form do not go together";
        if ((in[4] != nullptr) != have || (in[5] != nullptr) != (have && moments)) return "vr_filter_probe: the history's arrays are not all set or all null";
        if ((p[7] > 0.0f) != (out[4] != nullptr)) return "vr_filter_probe: the scratch read-back goes with tau > 0, and only with it";
        break;
    }
    case 3: if (i0 < 1.0f || i0 > (float)vr::kExpectedMaxRays) return "vr_filter_probe: rays must be in 1..4"; break;
    case 7:
        if (i0 < 1.0f || i0 > (float)vr::kExpectedMaxRays) return "vr_filter_probe: rays must be in 1..4";
        if (i1 < (float)vr::kUpsampleMinFactor || i1 > (float)vr::kUpsampleMaxFactor) return "vr_filter_probe: f must be in 2..4";
        break;
    case 8: {
        if (i0 < 1.0f || i0 > 65536.0f) return "vr_filter_probe: the number of tiles must be in 1..65536";
        const int32_t* ids = static_cast<const int32_t*>(in[2]);
        const int32_t tiles = vr::tile_count(W, H);
        for (int32_t k = 0; k < (int32_t)i0; ++k) if (ids[k] < 0 || ids[k] >= tiles) return "vr_filter_probe: a tile id outside the frame";
        break;
    }
    default: break;
    }
    return nullptr;
}
int vr_filter_probe(vr_renderer* r, int stage, int W, int H, const void* const* in, float* const* out, const float* params) {
    NEED(r);
    if (const char* why = filter_probe_error(stage, W, H, in, out, params)) return fail(VR_ERR_ARG, why);
    NEED_DEVICE();
    if ((stage == 3 || stage == 7) && (W != r->impl.resolution.x || H != r->impl.resolution.y))
        return fail(VR_ERR_ARG, "vr_filter_probe: resolve and upsample read the renderer's scene and need W x H to be its resolution");
    return guard([&] { use_device(r); r->impl.filter_probe(stage, W, H, in, out, params); });
}

int vr_write_brick_from_dense(const float* voxels, int nx, int ny, int nz, const float* transform, const char* path) {
    if (!voxels || !path || nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_ARG, "bad arguments");
    return guard([&] {
        auto d = std::make_shared<vr::DenseGrid>((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, voxels);
        if (transform) memcpy(d->transform.m, transform, 64);
        vr::Volume::to_brick_grid(d)->write(path);
    });
}

// writes this build's ".dense" container (grids.cpp): u8 voxels with value = lo + u8 / 255 * (hi - lo)
int vr_write_dense(const uint8_t* voxels, int nx, int ny, int nz, float lo, float hi, const float* transform, const char* path) {
    if (!voxels || !path || nx <= 0 || ny <= 0 || nz <= 0) return fail(VR_ERR_ARG, "bad dense grid arguments");
    return guard([&] {
        vr::mat4 t;
        if (transform) memcpy(t.m, transform, 64);
        vr::write_dense_file(path, t, (uint32_t)nx, (uint32_t)ny, (uint32_t)nz, lo, hi, voxels);
    });
}

int vr_encode_dense_stats(const float* voxels, int nx, int ny, int nz, uint32_t nb[3], uint64_t* counter, float mm[2]) {
    if (!voxels || !nb || !counter || !mm) return fail(VR_ERR_ARG, "null argument");
    return guard([&] {
        auto d = std::make_shared<vr::DenseGrid>((uint32_t)nx, (uint32_t)ny, (uint32_t)nz, voxels);
        auto b = vr::Volume::to_brick_grid(d);
        nb[0] = b->n_bricks.x; nb[1] = b->n_bricks.y; nb[2] = b->n_bricks.z;
        *counter = b->brick_counter;
        mm[0] = b->min_maj.first; mm[1] = b->min_maj.second;
    });
}

}  // extern "C"
