// tests/hostkernel/variant_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The product's rule "which compiled path-tracing kernel serves a scene" (volren_amd/csrc/vr_variant.h) compiled alone for the host, so that
// tests/test_variant_rule_host.py can hold it to a table of expected answers.  The scene comes as the few fields the rule reads; the views' pointers are flags
// (set or null) that nothing dereferences, so no table is allocated.
#include <cstddef>      // size_t, which vr_scene.h takes from whoever includes it

#include "../../volren_amd/csrc/vr_variant.h"

using namespace vr;

extern "C" {

struct vh_grid { int32_t dense, atlas_f32, maj_blocked, nb[3], mshift[3], dim[3], dblk[2]; };
struct vh_scene { int32_t integrator, use_tf, has_emission, env_div_safe, paired; float density_scale; vh_grid density, emission; };

static GridView view_of(const vh_grid& g) {
    static const uint16_t some_voxels = 0;
    static const float some_floats = 0.0f;
    GridView v{};
    v.dense = g.dense ? &some_voxels : nullptr;
    v.atlas_f32 = g.atlas_f32 ? &some_floats : nullptr;
    v.maj_blocked = g.maj_blocked;
    for (int i = 0; i < 3; ++i) { v.nb[i] = g.nb[i]; v.mshift[i] = g.mshift[i]; v.dim[i] = g.dim[i]; }
    for (int i = 0; i < 2; ++i) v.dblk[i] = g.dblk[i];
    return v;
}

// out: PathtraceKernel's variant, reason, instance, item_integrator, samples_per_unit, wide, reads_seed_table; then [7] pathtrace_scene_reasons and
// [8] scene_pairs_atlases, the predicate by which the harness scenes pair their atlases (host_kernel.cpp build_lane_scene, probe_host.cpp hp_scene_create)
void vh_kernel_of(const vh_scene* s, int force_wide, int instrumented, int32_t out[9]) {
    SceneParams P{};
    P.u.integrator = s->integrator; P.u.use_tf = s->use_tf; P.u.has_emission = s->has_emission; P.u.vol_density_scale = s->density_scale;
    P.env_div_safe = s->env_div_safe; P.paired = s->paired;
    P.density = view_of(s->density);
    P.emission = view_of(s->emission);
    const PathtraceKernel k = pathtrace_kernel_of(P, force_wide != 0, instrumented != 0);
    out[0] = k.variant; out[1] = k.reason; out[2] = k.instance; out[3] = k.item_integrator; out[4] = k.samples_per_unit; out[5] = k.wide ? 1 : 0; out[6] = k.reads_seed_table ? 1 : 0;
    out[7] = pathtrace_scene_reasons(P);
    out[8] = scene_pairs_atlases(P) ? 1 : 0;
}
}
