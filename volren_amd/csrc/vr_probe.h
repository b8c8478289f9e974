// vr_probe.h -- test hook: every scene-data lookup of the path tracer, one item at a time.
//
// A probe item is four 32-bit words in and probe_out_words(what) floats out.  probe_item calls THE inline functions of vr_trace.h that the
// path-tracing kernels and the feature kernel call, in the compile-time forms those kernels instantiate (vr_pathtrace.hip: TraceCfg<TF, 0, 0, 0>,
// <TF, 0, 0, 1>, <TF, 0, 1, 0>, <TF, 0, 1, 0, 1> and the run-time <TF, 2, 2, 2, 2>, which is also the form of feature_pixel), on a SceneParams
// filled as a launch fills it (RendererHIP::probe).  Host/device like vr_denoise.h and vr_adaptive.h: probe_kernel (vr_probe.hip) runs it on the
// device, tests/hostkernel/probe_host.cpp on the CPU -- the same text, against the same oracle.  Nothing here is on a render's path.
//
//   what            words in                          floats out                 form
//   PROBE_VOXEL     grid (0 density, 1 emission),     value                      DENSE + 3 PAIR: (0,0) (1,0) (2,0) and, on a scene with a paired atlas,
//                   x, y, z (int32)                                              (0,1) for the density grid, (0,2) for the emission grid
//   PROBE_TRILINEAR grid, x, y, z (float, index       density_scale * value      DENSE + 3 PAIR + 6 F32; PAIR 0 | 1 (density grid of a paired scene);
//                   space)                                                       F32 1: the decoded float atlas (must exist), 0: the byte atlas
//   PROBE_MAJORANT  x, y, z (float), mip (int32)      majorant                   TF + 2 DENSE + 6 MAJB + 18 CLEAN; (DENSE, MAJB) = (0,0) (1,0) (0,1) (2,2);
//                                                                                CLEAN (not with (2,2)): finite positions below 2^20 only
//   PROBE_IMPORTANCE x, y, mip (int32), -             importance                 0 imp_fetch, 1 env_average_importance as a launch passes it,
//                                                                                2 env_average_importance fetched (env_avg_w_set = 0)
//   PROBE_TEXEL     u, v (float), -, -                r, g, b                    0 float map, 1 compact map (must exist)
//   PROBE_SKY       direction x, y, z (float), -      r, g, b                    0
//   PROBE_LIGHT     r0, r1 (float), -, -              w_i, Le, pdf (7)           0 sample_environment<true, true> (needs env_div_safe), 1 <false, false>
//   PROBE_TF        density (float), -, -, -          r, g, b, a                 0 (needs a LUT)
//   PROBE_CUBIC     grid, x, y, z (float, index       value, gx, gy, gz          DENSE: 0 | 1 | 2.  vr_cubic.h cubic_lookup: the raw cubic B-spline value (no
//                   space)                            (voxel units)              density scale) and its gradient, from the byte atlas or the fp16 voxels
//
// probe_form_error says why a scene cannot serve a form (nullptr: it can); probe_items_error checks what would index outside a table.
#pragma once

#include "vr_cubic.h"
#include "vr_trace.h"

namespace vr {

enum ProbeWhat { PROBE_VOXEL = 0, PROBE_TRILINEAR, PROBE_MAJORANT, PROBE_IMPORTANCE, PROBE_TEXEL, PROBE_SKY, PROBE_LIGHT, PROBE_TF, PROBE_CUBIC, PROBE_COUNT };
constexpr int32_t kProbeInWords = 4;
VR_HD int32_t probe_out_words(int32_t what) {
    return what == PROBE_LIGHT ? 7 : ((what == PROBE_TF || what == PROBE_CUBIC) ? 4 : ((what == PROBE_TEXEL || what == PROBE_SKY) ? 3 : 1));
}

struct ProbeForm { int32_t dense, pair, majb, f32; bool tf, clean; };
inline ProbeForm probe_decode_form(int32_t what, int32_t form) {
    ProbeForm f{ 0, 0, 0, 0, false, false };
    if (what == PROBE_VOXEL) { f.dense = form % 3; f.pair = form / 3; }
    else if (what == PROBE_CUBIC) f.dense = form % 3;
    else if (what == PROBE_TRILINEAR) { f.dense = form % 3; f.pair = (form / 3) % 2; f.f32 = form / 6; }
    else if (what == PROBE_MAJORANT) { f.tf = (form & 1) != 0; f.dense = (form >> 1) % 3; f.majb = (form / 6) % 3; f.clean = form / 18 != 0; }
    return f;
}

// P: the SceneParams of the next launch (RendererHIP::fill_params).  nullptr, or why `form` of probe `what` cannot run on it.
inline const char* probe_form_error(const SceneParams& P, int32_t what, int32_t form) {
    if (what < 0 || what >= PROBE_COUNT) return "unknown probe";
    if (form < 0) return "negative form";
    const ProbeForm f = probe_decode_form(what, form);
    const bool dense_grid = P.density.dense != nullptr;
    switch (what) {
    case PROBE_VOXEL:
    case PROBE_TRILINEAR:
        if (what == PROBE_VOXEL ? form >= 9 : form >= 12) return "form out of range";
        if (f.pair != 0 && f.dense != 0) return "no kernel reads a paired atlas in a DENSE form other than 0";
        if (f.pair != 0 && !P.paired) return "PAIR form on a scene without a paired atlas";
        if (f.dense == 0 && dense_grid) return "DENSE = 0 form on a dense density grid";
        if (f.dense == 1 && !dense_grid) return "DENSE = 1 form on a brick density grid";
        if (f.f32 && (dense_grid || !P.density.atlas_f32)) return "no decoded float atlas (needs a brick grid, a LUT and tf_float_atlas)";
        return nullptr;
    case PROBE_MAJORANT:
        if (form >= 36) return "form out of range";
        if (!((f.dense == 0 && f.majb == 0) || (f.dense == 1 && f.majb == 0) || (f.dense == 0 && f.majb == 1) || (f.dense == 2 && f.majb == 2)))
            return "no kernel is compiled for this (DENSE, MAJB)";
        if (f.clean && f.dense == 2) return "the run-time variant has no CLEAN form";
        if (f.tf != (P.u.use_tf != 0)) return "TF form does not match the scene (a kernel's TF instance is chosen by use_tf)";
        if (f.dense == 0 && dense_grid) return "DENSE = 0 form on a dense density grid";
        if (f.dense == 1 && !dense_grid) return "DENSE = 1 form on a brick density grid";
        if (f.majb != 2 && (f.majb == 1) != (P.density.maj_blocked != 0)) return "MAJB form does not match the layout the table is built in";
        return nullptr;
    case PROBE_IMPORTANCE: return form > 2 ? "form out of range" : nullptr;
    case PROBE_TEXEL:
        if (form > 1) return "form out of range";
        return (form == 1 && !P.env_rgbe) ? "the environment map has no compact form" : nullptr;
    case PROBE_SKY: return form != 0 ? "form out of range" : nullptr;
    case PROBE_LIGHT:
        if (form > 1) return "form out of range";
        return (form == 0 && !P.env_div_safe) ? "the div_core sampler on a warp table that failed the division check (env_div_safe = 0)" : nullptr;
    case PROBE_TF:
        if (form != 0) return "form out of range";
        return P.u.use_tf ? nullptr : "no transfer function bound";
    case PROBE_CUBIC:
        if (form >= 3) return "form out of range";
        if (f.dense == 0 && dense_grid) return "DENSE = 0 form on a dense density grid";
        if (f.dense == 1 && !dense_grid) return "DENSE = 1 form on a brick density grid";
        return nullptr;
    }
    return "unknown probe";
}

// what an item must satisfy for its lookups to stay inside the tables (everything else -- NaN, infinities, any integer -- is the accessor's own business)
inline const char* probe_items_error(const SceneParams& P, int32_t what, int32_t form, const uint32_t* in, size_t n) {
    const ProbeForm f = probe_decode_form(what, form);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t* w = in + kProbeInWords * i;
        if (what == PROBE_CUBIC) {
            if (w[0] > 1u) return "grid must be 0 (density) or 1 (emission)";
            if (w[0] == 1u && !P.u.has_emission) return "no emission grid";
            if (w[0] == 1u && f.dense == 1) return "only the density grid has a compiled-in dense form";
            if (w[0] == 1u && f.dense == 0 && P.emission.dense) return "DENSE = 0 form on a dense emission grid";
        } else if (what == PROBE_VOXEL || what == PROBE_TRILINEAR) {
            if (w[0] > 1u) return "grid must be 0 (density) or 1 (emission)";
            if (w[0] == 1u && !P.u.has_emission) return "no emission grid";
            if (f.pair != 0 && w[0] != (what == PROBE_VOXEL ? (uint32_t)f.pair - 1u : 0u)) return "PAIR 1 reads the density grid, PAIR 2 the emission grid";
            if (w[0] == 1u && (f.f32 || f.dense == 1)) return "only the density grid has a decoded float atlas or a compiled-in dense form";
            if (w[0] == 1u && f.dense == 0 && P.emission.dense) return "DENSE = 0 form on a dense emission grid";
        } else if (what == PROBE_MAJORANT) {
            if (w[3] > 3u) return "mip must be 0..3 (the table has four levels)";
            if (f.clean)
                for (int k = 0; k < 3; ++k) { const float x = u2f(w[k]); if (!(abs_(x) < kCleanBound)) return "CLEAN form: positions must be finite and below 2^20"; }
        } else if (what == PROBE_IMPORTANCE && form == 0) {
            if ((int32_t)w[2] < 0 || (int32_t)w[2] > P.u.env_imp_base_mip) return "mip outside the pyramid";
        }
    }
    return nullptr;
}

template <int DENSE, int PAIR>
VR_HD float probe_voxel(const GridView& g, int32_t x, int32_t y, int32_t z) {
    const TapAddr a = tap_addr<DENSE>(g, x, y, z);
    return tap_value<DENSE>(g, tap_load<DENSE, PAIR>(g, a), a.in);
}
template <int DENSE, int PAIR>
VR_HD float probe_trilinear(const SceneParams& P, const GridView& g, v3 ipos) {
    TriIO io;
    trilinear_prep<DENSE>(g, ipos, io);
    trilinear_load<DENSE, PAIR>(g, io);
    return P.u.vol_density_scale * trilinear_value<DENSE>(g, io);
}
template <bool TF, int DENSE, int MAJB, bool CLEAN>
VR_HD float probe_majorant(const SceneParams& P, v3 ipos, int32_t mip) {
    if (!CLEAN) return majorant_at<TF, DENSE, MAJB>(P, ipos, mip);
    const int32_t idx = majorant_index<DENSE, MAJB, CLEAN>(P.density, ipos, mip);      // as march_prep / march_load / march_finish do on a clean segment
    return majorant_value<TF>(P, majorant_fetch<TF>(P.density, idx));
}

// one item.  `P` by reference: the forms that need a changed view (byte atlas, float map, fetched average) work on a copy of the few fields they change
VR_HD void probe_item(const SceneParams& P, int32_t what, int32_t form, const uint32_t* w, float* out) {
    const float fx = u2f(w[0]), fy = u2f(w[1]), fz = u2f(w[2]);
    switch (what) {
    case PROBE_VOXEL: {
        const GridView& g = w[0] ? P.emission : P.density;
        const int32_t x = (int32_t)w[1], y = (int32_t)w[2], z = (int32_t)w[3];
        switch (form) {
        case 0: out[0] = probe_voxel<0, 0>(g, x, y, z); break;
        case 1: out[0] = probe_voxel<1, 0>(g, x, y, z); break;
        case 2: out[0] = probe_voxel<2, 0>(g, x, y, z); break;
        case 3: out[0] = probe_voxel<0, 1>(g, x, y, z); break;
        case 6: out[0] = probe_voxel<0, 2>(g, x, y, z); break;
        default: out[0] = nan_(); break;
        }
        break;
    }
    case PROBE_TRILINEAR: {
        GridView g = w[0] ? P.emission : P.density;
        if (form < 6) g.atlas_f32 = nullptr;                 // the byte atlas, as a launch without a decoded atlas reads it
        const v3 p{ u2f(w[1]), u2f(w[2]), u2f(w[3]) };
        switch (form % 6) {
        case 0: out[0] = probe_trilinear<0, 0>(P, g, p); break;
        case 1: out[0] = probe_trilinear<1, 0>(P, g, p); break;
        case 2: out[0] = probe_trilinear<2, 0>(P, g, p); break;
        case 3: out[0] = probe_trilinear<0, 1>(P, g, p); break;
        default: out[0] = nan_(); break;
        }
        break;
    }
    case PROBE_MAJORANT: {
        const v3 p{ fx, fy, fz };
        const int32_t mip = (int32_t)w[3];
#define VR_PROBE_MAJ(TF, DENSE, MAJB, CLEAN) case ((TF ? 1 : 0) + 2 * DENSE + 6 * MAJB + (CLEAN ? 18 : 0)): out[0] = probe_majorant<TF, DENSE, MAJB, CLEAN>(P, p, mip); break;
        switch (form) {
        VR_PROBE_MAJ(false, 0, 0, false) VR_PROBE_MAJ(true, 0, 0, false) VR_PROBE_MAJ(false, 0, 0, true) VR_PROBE_MAJ(true, 0, 0, true)
        VR_PROBE_MAJ(false, 1, 0, false) VR_PROBE_MAJ(true, 1, 0, false) VR_PROBE_MAJ(false, 1, 0, true) VR_PROBE_MAJ(true, 1, 0, true)
        VR_PROBE_MAJ(false, 0, 1, false) VR_PROBE_MAJ(true, 0, 1, false) VR_PROBE_MAJ(false, 0, 1, true) VR_PROBE_MAJ(true, 0, 1, true)
        VR_PROBE_MAJ(false, 2, 2, false) VR_PROBE_MAJ(true, 2, 2, false)
        default: out[0] = nan_(); break;
        }
#undef VR_PROBE_MAJ
        break;
    }
    case PROBE_IMPORTANCE:
        if (form == 0) out[0] = imp_fetch(P, (int32_t)w[0], (int32_t)w[1], (int32_t)w[2]);
        else if (form == 1) out[0] = env_average_importance(P);
        else { SceneParams Q; Q.u.env_imp_base_mip = P.u.env_imp_base_mip; Q.impmap = P.impmap; Q.imp_dim = P.imp_dim; Q.env_avg_w_set = 0; Q.env_avg_w = 0.0f; out[0] = env_average_importance(Q); }
        break;
    case PROBE_TEXEL: {
        SceneParams Q;                                        // env_texture reads these four fields only (as impmap_base_kernel relies on)
        Q.envmap = P.envmap; Q.env_rgbe = form == 1 ? P.env_rgbe : nullptr; Q.env_w = P.env_w; Q.env_h = P.env_h;
        const v3 c = env_texture(Q, fx, fy);
        out[0] = c.x; out[1] = c.y; out[2] = c.z;
        break;
    }
    case PROBE_SKY: {
        const v3 c = lookup_environment(P, v3{ fx, fy, fz });
        out[0] = c.x; out[1] = c.y; out[2] = c.z;
        break;
    }
    case PROBE_LIGHT: {
        v3 wi, Le; float pdf;
        if (form == 0) sample_environment<true, true>(P, fx, fy, wi, Le, pdf);
        else sample_environment<false, false>(P, fx, fy, wi, Le, pdf);
        out[0] = wi.x; out[1] = wi.y; out[2] = wi.z; out[3] = Le.x; out[4] = Le.y; out[5] = Le.z; out[6] = pdf;
        break;
    }
    case PROBE_TF: tf_lookup(P, fx, out); break;
    case PROBE_CUBIC: {
        const GridView& g = w[0] ? P.emission : P.density;
        const v3 p{ u2f(w[1]), u2f(w[2]), u2f(w[3]) };
        v3 gr{ 0.0f, 0.0f, 0.0f };
        out[0] = nan_();
        switch (form) {
        case 0: cubic_lookup<0>(g, p, out[0], gr); break;
        case 1: cubic_lookup<1>(g, p, out[0], gr); break;
        case 2: cubic_lookup<2>(g, p, out[0], gr); break;
        default: break;
        }
        out[1] = gr.x; out[2] = gr.y; out[3] = gr.z;
        break;
    }
    default: break;
    }
}

}  // namespace vr
