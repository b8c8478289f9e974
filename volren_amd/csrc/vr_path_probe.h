// vr_path_probe.h -- test hook: the per-path layer of vr_trace.h, one item at a time -- the code that turns a pixel into a ray, a ray into a segment and a
// segment into a collision.  Like vr_probe.h one layer down: path_probe_item calls THE inline functions of vr_trace.h that the path-tracing kernels call, in
// the compile-time forms vr_pathtrace.hip instantiates, on a SceneParams filled as a launch fills it (RendererHIP::path_probe).  Host/device: path_probe_kernel
// and path_segment_kernel (vr_probe.hip) run it on the device, tests/hostkernel/path_probe_host.cpp on the CPU -- the same text, against the same oracle
// (oracle/volren_oracle.h orc_batch_rng ... orc_batch_segment, which state the item layouts).  Nothing here is on a render's path.
//
// Items are 32-bit words in and out: floats as their bits, integers as they are.
//   kind          words in                                   words out                                                     form
//   PATH_RNG      state, v0, v1, seed, W, px, py, smp        rng(state), state after, state after rng_skip9,               0
//                                                            tea32(v0, v1), path_seed(seed, W, px, py, smp)
//   PATH_CAMERA   px, py, smp, -                             do_new's direction (3), the RNG state after the two jitter    0
//                                                            draws; under the scene's camera, seed and resolution
//   PATH_BOX      pos (3), dir (3)                           intersect_box: hit, near, far                                 0
//   PATH_PHASE    cos, g, dir (3), r0, r1, a, b              phase_hg(cos, g), sample_phase_hg(dir, g, r0, r1) (3),        0
//                                                            power_heuristic(a, b)
//   PATH_DDA      p (3), ri (3), mip                         step_dda                                                      0 general, 1 CLEAN (p below 2^21, |ri| above 2^-20, no NaN)
//   PATH_SEGMENT  pos (3), dir (3), RNG state,               status, t, tau, mipq, RNG state after, tentative collisions,  0..6: the compiled instance, in the order of
//                 0 camera / scatter | 1 shadow segment      Tr, colour of the real collision (3, LUT), radiance gathered  PathtraceKernel::instance (vr_variant.h)
//                                                            with throughput 1 (3, emission grid), seg_clean
// status: 0 the ray missed the box, 1 the segment ended without a real collision (shadow: it left the box), 2 real collision (shadow: the roulette ended it),
// 3 the item ran out of passes or stalled.
//
// PATH_SEGMENT runs hot_init, begin_segment<K> and then the passes of the scheduler's hot pair (vr_pathtrace.h hot_pair), each in the form CLEAN = seg_clean(h) of
// the item: march_prep / march_load[_reuse] / march_finish, collide_prep / collide_load / collide_finish<K, Cold, true, EARLY> with the scheduler's rule for EARLY.
// The loop is bounded: at most kPathSegmentPasses passes (a pass is at most two DDA steps or one collision, so whatever the oracle finishes within
// ORC_SEGMENT_BUDGET iterations ends here), and a march pass that changes neither t, tau nor mipq ends the item, as in feature_sample.
#pragma once

#include "vr_trace.h"
#include "vr_variant.h"

namespace vr {

enum PathProbeKind { PATH_RNG = 0, PATH_CAMERA, PATH_BOX, PATH_PHASE, PATH_DDA, PATH_SEGMENT, PATH_COUNT };
constexpr int32_t kPathSegmentBudget = 4096;                        // the oracle's ORC_SEGMENT_BUDGET (tests/test_path_probes_host.py holds the two together)
constexpr int32_t kPathSegmentPasses = 2 * kPathSegmentBudget;
VR_SCENE_HD int32_t path_probe_in_words(int32_t kind) { return kind == PATH_RNG ? 8 : (kind == PATH_CAMERA ? 4 : (kind == PATH_BOX ? 6 : (kind == PATH_PHASE ? 9 : (kind == PATH_DDA ? 7 : 8)))); }
VR_SCENE_HD int32_t path_probe_out_words(int32_t kind) { return kind == PATH_RNG ? 5 : (kind == PATH_CAMERA ? 4 : (kind == PATH_BOX ? 3 : (kind == PATH_PHASE ? 5 : (kind == PATH_DDA ? 1 : 14)))); }

// P: the SceneParams of the next launch, with the paired views where the scene has them.  nullptr, or why `form` of `kind` cannot run on it.  A segment form is
// the compiled instance: the one the scene's launch runs (pathtrace_kernel_of), its wide twin (what the tuning's wide_addressing forces) and the run-time
// instance, which is correct for every scene.
inline const char* path_probe_form_error(const SceneParams& P, int32_t kind, int32_t form) {
    if (kind < 0 || kind >= PATH_COUNT) return "unknown kind";
    if (form < 0) return "negative form";
    if (kind == PATH_DDA) return form > 1 ? "form out of range" : nullptr;
    if (kind != PATH_SEGMENT) return form != 0 ? "form out of range" : nullptr;
    if (form >= kPtInstances) return "form out of range";
    const PathtraceKernel k = pathtrace_kernel_of(P, false, false);
    if (form == k.instance || form == kPtInstances - 1) return nullptr;
    if (k.variant <= 1 && !k.wide && form == k.instance + 1) return nullptr;
    if (k.reason & VR_VARIANT_INTEGRATOR) return "the scene's launch runs the run-time instance (6): an integrator other than the DDA trackers";
    if (k.reason & VR_VARIANT_ENV_DIVISION) return "the scene's launch runs the run-time instance (6): the environment's warp table failed the division check";
    if (k.reason & VR_VARIANT_DENSITY_SCALE) return "the scene's launch runs the run-time instance (6): density scale outside [2^-16, 2^24]";
    if (k.reason & VR_VARIANT_GRID_FORMS) return "the scene's launch runs the run-time instance (6): grids without a compiled form or a paired atlas";
    if (k.variant <= 1 && k.wide && form == k.instance - 1) return "a table of 4 GiB or more: the scene's launch runs the instance with 64-bit gather addresses";
    return "the scene's launch runs another instance (its grids are of another kind)";
}
inline const char* path_probe_items_error(const SceneParams& P, int32_t kind, int32_t form, const uint32_t* in, size_t n) {
    const int32_t k = path_probe_in_words(kind);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t* w = in + (size_t)k * i;
        if (kind == PATH_CAMERA) {
            if (w[0] >= (uint32_t)P.u.resolution[0] || w[1] >= (uint32_t)P.u.resolution[1]) return "pixel outside the frame";
        } else if (kind == PATH_DDA) {
            if (w[6] > 3u) return "mip must be 0..3";
            if (form == 1) {
                for (int j = 0; j < 3; ++j) { const float x = u2f(w[j]); if (!(abs_(x) < 2.0f * kCleanBound)) return "CLEAN form: positions must be finite and below 2^21"; }
                // (seg_clean: |idir| < 2^20 on every axis, so a reciprocal is larger than 2^-20 in modulus, or infinite)
                for (int j = 3; j < 6; ++j) { const float x = u2f(w[j]); if (!(abs_(x) > 1.0f / kCleanBound)) return "CLEAN form: reciprocals above 2^-20 in modulus, no NaN"; }
            }
        } else if (kind == PATH_SEGMENT) {
            if (w[7] > 1u) return "segment kind must be 0 (camera / scatter) or 1 (shadow)";
        }
    }
    return nullptr;
}

struct PathCold {
    float v[C_COUNT];
    VR_HD float ld(int32_t f) const { return v[f]; }
    VR_HD void st(int32_t f, float x) { v[f] = x; }
};

// the scheduler's rule for the early collision tail (vr_pathtrace.h collide_tail_early<K, false>: no statistics), restated because this header is also compiled for
// the host, where the scheduler's is not; vr_probe.hip holds the two equal for every instance with a static_assert, experiment builds (VR_COLLIDE_EARLY) included
template <class K> constexpr bool path_collide_early() {
#ifdef VR_COLLIDE_EARLY
    return K::global == 0 && VR_COLLIDE_EARLY != 0;
#else
    return !K::tf && K::global == 0 && K::emission == 0 && K::dense == 0 && K::a32 && !VR_FAST_DEVICE;
#endif
}

template <class K, bool CLEAN>
VR_HD void path_march_pass(Hot& h, const SceneParams& P) {
    MarchIO mio;
    march_idle(mio);
    march_prep<K::dense, K::majb, CLEAN>(h, P, mio);
    if constexpr (K::maj_reuse) march_load_reuse<K::tf, K::a32>(P, mio, h);
    else march_load<K::tf, K::a32>(P, mio);
    march_finish<K::tf, K::maj_reuse, CLEAN>(h, P, mio);
}
template <class K, bool CLEAN>
VR_HD void path_collide_pass(Hot& h, PathCold& c, const SceneParams& P) {
    CollideIO<K> cio;
    collide_idle<K>(cio);
    collide_prep<K, CLEAN>(h, P, P, cio);
    collide_load<K>(P, P, cio);
    collide_finish<K, PathCold, true, path_collide_early<K>()>(h, c, P, P, cio, P.tf_lut);
}

template <class K>
VR_HD void path_segment(const SceneParams& P, const uint32_t* w, uint32_t* out) {
    Hot h;
    hot_init(h);
    PathCold c;
    for (int32_t i = 0; i < C_COUNT; ++i) c.v[i] = 0.0f;
    h.seed = w[6];
    h.ethr = v3{ 1.0f, 1.0f, 1.0f };
    const int32_t shadow = (int32_t)w[7];
    uint32_t n_coll = 0u;
    bool killed = false, clean = false;
    int32_t status = 0;
    if (begin_segment<K>(h, P, v3{ u2f(w[0]), u2f(w[1]), u2f(w[2]) }, v3{ u2f(w[3]), u2f(w[4]), u2f(w[5]) }, shadow)) {
        clean = seg_clean(h);
        for (int32_t pass = 0; pass < kPathSegmentPasses && (h.state == ST_MARCH || h.state == ST_COLLIDE); ++pass) {
            if (h.state == ST_MARCH) {
                const float t0 = h.t, tau0 = h.tau;
                const int32_t mip0 = h.mipq;
                if (seg_clean(h)) path_march_pass<K, true>(h, P);
                else path_march_pass<K, false>(h, P);
                if (h.state == ST_MARCH && h.t == t0 && h.tau == tau0 && h.mipq == mip0) break;      // stalled: t + dt == t
            } else {
                ++n_coll;
                if (seg_clean(h)) path_collide_pass<K, true>(h, c, P);
                else path_collide_pass<K, false>(h, c, P);
                // a shadow segment's roulette leaves Tr = +0 exactly, and a ray that leaves the box never does: a Tr of 0 always meets prob = 1
                killed = shadow != 0 && h.state == ST_POSTNEE && h.Tr == 0.0f;
            }
        }
        if (h.state == ST_MARCH || h.state == ST_COLLIDE) status = 3;
        else if (shadow) status = killed ? 2 : 1;
        else status = h.state == ST_NEE ? 2 : 1;
    }
    out[0] = (uint32_t)status; out[1] = f2u(h.t); out[2] = f2u(h.tau); out[3] = (uint32_t)h.mipq; out[4] = h.seed; out[5] = n_coll; out[6] = f2u(h.Tr);
    out[7] = f2u(c.v[C_COL]); out[8] = f2u(c.v[C_COL + 1]); out[9] = f2u(c.v[C_COL + 2]);
    out[10] = f2u(h.eL.x); out[11] = f2u(h.eL.y); out[12] = f2u(h.eL.z);
    out[13] = clean ? 1u : 0u;
}
// form: the compiled instance (vr_pathtrace.hip: variant 0, 0 wide, 1, 1 wide, 2, 4, 3)
template <int FORM, bool TF> struct PathInstance;
template <bool TF> struct PathInstance<0, TF> { using K = TraceCfg<TF, 0, 0, 0, 0, true>; };
template <bool TF> struct PathInstance<1, TF> { using K = TraceCfg<TF, 0, 0, 0, 0, false>; };
template <bool TF> struct PathInstance<2, TF> { using K = TraceCfg<TF, 0, 0, 1, 0, true>; };
template <bool TF> struct PathInstance<3, TF> { using K = TraceCfg<TF, 0, 0, 1, 0, false>; };
template <bool TF> struct PathInstance<4, TF> { using K = TraceCfg<TF, 0, 1, 0, 0, false>; };
template <bool TF> struct PathInstance<5, TF> { using K = TraceCfg<TF, 0, 1, 0, 1, false>; };
template <bool TF> struct PathInstance<6, TF> { using K = TraceCfg<TF, 2, 2, 2, 2, false>; };
template <int FORM>
VR_HD void path_segment_form(const SceneParams& P, const uint32_t* w, uint32_t* out) {
    if (P.u.use_tf) path_segment<typename PathInstance<FORM, true>::K>(P, w, out);
    else path_segment<typename PathInstance<FORM, false>::K>(P, w, out);
}

// the scene-free kinds
VR_HD void path_probe_item(const SceneParams& P, int32_t kind, int32_t form, const uint32_t* w, uint32_t* out) {
    switch (kind) {
    case PATH_RNG: {
        uint32_t s = w[0];
        out[0] = f2u(rng(s)); out[1] = s;
        uint32_t s9 = w[0];
        rng_skip9(s9);
        out[2] = s9;
        out[3] = tea32(w[1], w[2]);
        out[4] = path_seed(w[3], (int32_t)w[4], (int32_t)w[5], (int32_t)w[6], (int32_t)w[7]);
        break;
    }
    case PATH_CAMERA: {
        // do_new itself, for the one item of a work unit that starts at the pixel.  It leaves the ray's direction in Hot::wdir (begin_segment's argument) and has
        // made one more draw -- begin_segment's free-flight draw of the DDA trackers -- when the ray hits the box (the lane then marches): that one step of the
        // LCG is taken back (s = (s' - c) a^-1 mod 2^32, a bijection) to report the state after the two jitter draws
        using K = TraceCfg<false, 0, 0, 2, 2, false>;
        Hot h;
        hot_init(h);
        PathCold c;
        for (int32_t i = 0; i < C_COUNT; ++i) c.v[i] = 0.0f;
        WorkUnit wu;
        wu.px0 = (int32_t)w[0]; wu.py0 = (int32_t)w[1]; wu.first_sample = (int32_t)w[2]; wu.n_items = 1; wu.base = 0u; wu.out = nullptr;
        do_new<K, PathCold, true>(h, c, P, wu, 0u);
        out[0] = f2u(h.wdir.x); out[1] = f2u(h.wdir.y); out[2] = f2u(h.wdir.z);
        out[3] = h.state == ST_MARCH ? (h.seed - 1013904223u) * 4276115653u : h.seed;
        break;
    }
    case PATH_BOX: {
        float tn = 0.0f, tf = 0.0f;
        out[0] = intersect_box(v3{ u2f(w[0]), u2f(w[1]), u2f(w[2]) }, v3{ u2f(w[3]), u2f(w[4]), u2f(w[5]) }, P.u.vol_bb_min, P.u.vol_bb_max, tn, tf) ? 1u : 0u;
        out[1] = f2u(tn); out[2] = f2u(tf);
        break;
    }
    case PATH_PHASE: {
        out[0] = f2u(phase_hg(u2f(w[0]), u2f(w[1])));
        const v3 d = sample_phase_hg(v3{ u2f(w[2]), u2f(w[3]), u2f(w[4]) }, u2f(w[1]), u2f(w[5]), u2f(w[6]));
        out[1] = f2u(d.x); out[2] = f2u(d.y); out[3] = f2u(d.z);
        out[4] = f2u(power_heuristic(u2f(w[7]), u2f(w[8])));
        break;
    }
    case PATH_DDA: {
        const v3 p{ u2f(w[0]), u2f(w[1]), u2f(w[2]) }, ri{ u2f(w[3]), u2f(w[4]), u2f(w[5]) };
        out[0] = f2u(form == 1 ? step_dda<true>(p, ri, (int32_t)w[6]) : step_dda<false>(p, ri, (int32_t)w[6]));
        break;
    }
    default: break;
    }
}

}  // namespace vr
