// tests/hostkernel/path_probe_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The per-path probes of volren_amd/csrc/vr_path_probe.h -- the header path_probe_kernel and path_segment_kernel run on the device -- compiled for the host, in the
// same forms, on a scene built from the oracle's arrays as the product builds its device copies (host_scene.h).  tests/test_path_probes_host.py compares every
// item with the oracle's batch forms, bit for bit.  Built with -DVR_HOST_TRACE: the sink below checks every majorant and tap access the lane code makes against the
// extent of the table it names and counts what falls outside (hpp_violations); the test asserts 0.  That is the range check of this layer.
#include <atomic>
#include <cstdio>

#include "../../volren_amd/csrc/vr_path_probe.h"
#include "host_scene.h"

using namespace vr;
using namespace hostscene;

namespace {
struct PathScene {
    HostScene S;
    SceneParams paired{};      // the views of the kernels compiled for the paired atlas; == S.P when the scene has none
};
int fail(char* err, int errlen, const char* why) {
    if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", why);
    return 1;
}
// the scene whose tables the accesses of the running hpp_probe are held to (one call at a time: the binding does not run two)
const PathScene* g_scene = nullptr;
std::atomic<long long> g_violations{ 0 }, g_accesses{ 0 };
thread_local long long t_accesses = 0;      // per thread, added up at the end of a call: an atomic per access would serialise the lanes
}  // namespace

namespace vr {
void host_trace(int32_t cls, const void* table, size_t a, size_t b) {
    const PathScene* ps = g_scene;
    if (!ps) return;
    ++t_accesses;
    bool ok = false;
    const HostScene& S = ps->S;
    if (cls == TR_MAJORANT) {
        // a: the cell's index; every view's float and fp16 tables have the same number of cells
        ok = table == (const void*)S.dg.majorant16.data() && a < S.dg.majorant16.size() && a < S.dg.majorant.size();
    } else if (cls == TR_TAP) {
        // a: brick record (or 4x4x4 block of a dense grid), b: voxel inside it
        // (a dense grid's view also carries the brick atlas of its descriptor, and tap_load names the view by it: the access goes to the dense voxels)
        if (!S.blocked.empty() && (table == (const void*)S.blocked.data() || table == (const void*)S.dg.atlas.data())) ok = b < 64u && a * 64u + b < S.blocked.size();
        else if (table == (const void*)S.dg.atlas.data()) ok = b < 512u && a < S.dg.recs.size();
        else if (!S.eg.atlas.empty() && table == (const void*)S.eg.atlas.data()) ok = b < 512u && a < S.eg.recs.size();
        else if (!S.paired.empty() && table == (const void*)S.paired.data()) ok = b < 512u && a < S.dg.recs.size() && (a + 1u) * (size_t)kPairBlockBytes <= S.paired.size();
    }
    if (!ok) g_violations.fetch_add(1, std::memory_order_relaxed);
}
}  // namespace vr

extern "C" {

int hpp_uniforms_size() { return (int)sizeof(Uniforms); }
// [0] the segment budget of the device code, [1] its pass bound
void hpp_constants(int out[2]) { out[0] = kPathSegmentBudget; out[1] = kPathSegmentPasses; }

// flags: host_scene.h HS_*; 8 = pair the atlases when the product would
void* hpp_scene_create(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                       const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int flags) {
    PathScene* ps = new PathScene;
    build_scene(ps->S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim, flags);
    ps->paired = ps->S.P;
    if ((flags & 8) && scene_pairs_atlases(ps->S.P)) {
        build_paired_atlas(ps->S.dg, ps->S.eg, ps->S.paired);
        ps->paired.density.atlas = ps->S.paired.data();
        ps->paired.emission.atlas = ps->S.paired.data();
        ps->paired.paired = 1;
    }
    return ps;
}
void hpp_scene_free(void* h) { delete static_cast<PathScene*>(h); }
// out: [0] paired, [1] decoded float atlas present, [2] the instance the scene's launch runs, [3] the reason mask
void hpp_scene_info(void* h, int out[4]) {
    const PathScene* ps = static_cast<const PathScene*>(h);
    const PathtraceKernel k = pathtrace_kernel_of(ps->paired, false, false);
    out[0] = ps->paired.paired; out[1] = ps->S.P.density.atlas_f32 != nullptr; out[2] = k.instance; out[3] = k.reason;
}
long long hpp_violations() { return g_violations.load(); }
long long hpp_accesses() { return g_accesses.load(); }

// 0 ok; 1: the scene cannot serve the form, or a bad item (err says why)
int hpp_probe(void* h, int kind, int form, const uint32_t* in, uint32_t* out, long long n, char* err, int errlen) {
    const PathScene* ps = static_cast<const PathScene*>(h);
    if (const char* why = path_probe_form_error(ps->paired, kind, form)) return fail(err, errlen, why);
    if (const char* why = path_probe_items_error(ps->paired, kind, form, in, (size_t)n)) return fail(err, errlen, why);
    const SceneParams& P = (kind == PATH_SEGMENT && (form == 4 || form == 5)) ? ps->paired : ps->S.P;      // as RendererHIP::path_probe picks the views
    const size_t ki = (size_t)path_probe_in_words(kind), ko = (size_t)path_probe_out_words(kind);
    g_scene = ps;
#pragma omp parallel
    {
    t_accesses = 0;
#pragma omp for schedule(dynamic, 64)
    for (long long i = 0; i < n; ++i) {
        const uint32_t* w = in + ki * (size_t)i;
        uint32_t* o = out + ko * (size_t)i;
        if (kind != PATH_SEGMENT) { path_probe_item(P, kind, form, w, o); continue; }
        switch (form) {
        case 0: path_segment_form<0>(P, w, o); break;
        case 1: path_segment_form<1>(P, w, o); break;
        case 2: path_segment_form<2>(P, w, o); break;
        case 3: path_segment_form<3>(P, w, o); break;
        case 4: path_segment_form<4>(P, w, o); break;
        case 5: path_segment_form<5>(P, w, o); break;
        default: path_segment_form<6>(P, w, o); break;
        }
    }
    g_accesses.fetch_add(t_accesses, std::memory_order_relaxed);
    }
    g_scene = nullptr;
    return 0;
}

}  // extern "C"
