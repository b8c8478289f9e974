// vr_variant.h -- which compiled path-tracing kernel serves a scene, and which views of the grids that kernel is handed: the one statement of the rule.
// Plain arithmetic on SceneParams, for the host compiler as well: the launch (vr_launch.hip), the renderer's marshalling (renderer.cpp), the C ABI's read-outs
// (capi.cpp) and the CPU test harness (tests/hostkernel) all ask here, and tests/test_variant_rule_host.py holds this file to a table of expected answers.
#pragma once

#include <stdint.h>

#include "vr_scene.h"

namespace vr {

// what sent a scene to the run-time variant (PathtraceKernel::reason, a mask; 0: nothing, the scene has a kernel of its own kind)
enum PathtraceVariantReason : int {
    VR_VARIANT_INTEGRATOR = 1,        // a global-majorant / ray-marching integrator was asked for
    VR_VARIANT_ENV_DIVISION = 2,      // the environment's warp table failed env_cdf_kernel's check (thresholds below 2^-76: vr_math.h div_core does not apply)
    VR_VARIANT_DENSITY_SCALE = 4,     // density scale outside [2^-16, 2^24] (the clean march divides by majorants without rescaling)
    VR_VARIANT_GRID_FORMS = 8         // emission grid with a dense grid on either side, or brick grids of different layouts (no paired atlas)
};
// the density scales the kernels of one scene kind take: the CLEAN form of the march divides by majorants = density_scale x an fp16 number (vr_trace.h march_finish)
constexpr float kDensityScaleMin = 1.0f / 65536.0f, kDensityScaleMax = 16777216.0f;

// The reasons that hold whatever the grids are.  0: a kernel of one scene kind may serve the scene -- and only then are two brick grids read from a paired atlas.
// (An environment whose warp table failed the check of env_cdf_kernel -- the kernels of one scene kind divide by vr_math.h div_core there -- goes to the run-time
// variant, which divides in full.)
VR_SCENE_HD int pathtrace_scene_reasons(const SceneParams& P) {
    int reason = 0;
    if (P.u.integrator != 0) reason |= VR_VARIANT_INTEGRATOR;
    if (!P.env_div_safe) reason |= VR_VARIANT_ENV_DIVISION;
    if (!(P.u.vol_density_scale >= kDensityScaleMin && P.u.vol_density_scale <= kDensityScaleMax)) reason |= VR_VARIANT_DENSITY_SCALE;
    return reason;
}
// these two grids can share a paired atlas (vr_scene.h): both in brick form, with the same brick layout.  Two GridViews, or whatever else says `dense` and `nb` of
// a grid: the renderer's own records, of which commit() asks before there is a view
template <class A, class B> VR_SCENE_HD bool grids_can_pair(const A& a, const B& b) {
    return VR_PAIRED_ATLAS && !a.dense && !b.dense && a.nb[0] == b.nb[0] && a.nb[1] == b.nb[1] && a.nb[2] == b.nb[2];
}
// ... and are read from one wherever it can be built: how the host harness decides it for its scenes (the renderer asks for its shared atlas instead: fill_params)
VR_SCENE_HD bool scene_pairs_atlases(const SceneParams& P) { return P.u.has_emission && grids_can_pair(P.density, P.emission) && pathtrace_scene_reasons(P) == 0; }

// Variants (vr_pathtrace.hip): 0 bricks, 1 dense fp16, 2 / 4 bricks + emission grid from a paired atlas (4: majorant levels 0-1 in 4x4x4-cell blocks), 3 everything
// decided at run time -- correct for every scene, an order of magnitude slower on some.  Units of 8 samples x 64 pixels, except on the dense-grid kernel, whose long
// paths (128 bounces, every camera ray scatters) fill the pools better from units of 4: c4 +1.3 %, c2 +-0, c3 -1 % (profiles/r2x_occupancy_recheck.txt) -- and,
// round 4, on the emission kernels: c5cloud +1 %, c5full +0.5 % (profiles/r4d_*)
constexpr int kPtVariants = 5, kPtInstances = 7;
VR_SCENE_HD int32_t pathtrace_unit_samples(int variant) { return (variant == 1 || variant == 2 || variant == 4) ? 4 : 8; }

// The answer.  variant: 0..4; reason: a mask of PathtraceVariantReason; instance: 0..6, the compiled instance -- variant 0 with 32-bit gather offsets, variant 0 wide,
// variant 1, variant 1 wide, variant 2, variant 4, variant 3; item_integrator: 2 or 3, the item kernel (vr_launch.hip) that serves the launch instead of the
// path-tracing kernel, 0: none does; samples_per_unit: the variant's default unit; wide: the instance forms 64-bit gather addresses; reads_seed_table: it reads a
// seed table (vr_pathtrace.h seed_request_point: the brick kernels without an emission grid, not their instrumented forms) -- for every other launch the renderer
// neither fills nor passes one
struct PathtraceKernel {
    int32_t variant, reason, instance, item_integrator, samples_per_unit;
    bool wide, reads_seed_table;
};
// force_wide: the tuning's wide_addressing; instrumented: the launch uses the STATS kernels
VR_SCENE_HD PathtraceKernel pathtrace_kernel_of(const SceneParams& P, bool force_wide, bool instrumented) {
    PathtraceKernel k;
    k.reason = pathtrace_scene_reasons(P);
    if (k.reason) k.variant = 3;
    else if (P.u.has_emission) {
        // (P.paired: the renderer found both conditions above to hold and the shared atlas in place -- RendererHIP::fill_params)
        const bool mixed = P.density.dense || P.emission.dense || (VR_PAIRED_ATLAS && !P.paired);
        if (mixed) k.reason |= VR_VARIANT_GRID_FORMS;
        k.variant = mixed ? 3 : (P.density.maj_blocked ? 4 : 2);
    } else k.variant = P.density.dense ? 1 : 0;
    // a kernel's 32-bit byte offsets reach every byte of a table smaller than 2^32 bytes (vr_scene.h grid_largest_table_bytes); variants 2, 3 and 4 have no such
    // build -- and serve every scene with an emission grid, so that only the density grid's tables are left to decide
    k.wide = force_wide || k.variant >= 2 || grid_largest_table_bytes(P.density, P.paired != 0, P.u.use_tf != 0) >= (1ull << 32);
    k.instance = k.variant <= 1 ? 2 * k.variant + (k.wide ? 1 : 0) : (k.variant == 2 ? 4 : (k.variant == 4 ? 5 : 6));
    k.item_integrator = (P.u.integrator == 3 || (P.u.integrator == 2 && P.u.use_tf)) ? P.u.integrator : 0;
    k.samples_per_unit = pathtrace_unit_samples(k.variant);
    k.reads_seed_table = k.item_integrator == 0 && !instrumented && k.variant == 0;
    return k;
}

}  // namespace vr
