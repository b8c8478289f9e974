// tests/hostkernel/probe_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The lookup probes of volren_amd/csrc/vr_probe.h -- the header probe_kernel runs on the device -- compiled for the host and run on a scene built from the
// oracle's arrays as the product builds its device copies (host_scene.h): the compact environment map, the warp table and its division check, the majorant
// tables in both layouts, the decoded float atlas and the paired atlas.  tests/test_lookups_host.py compares every probe with the oracle, bit for bit, and
// runs this file under UBSan: the only place the forms PAIR = 1, 2 and MAJB = 0, 1 can meet a sanitizer.
#include <cstdio>

#include "../../volren_amd/csrc/vr_probe.h"
#include "../../volren_amd/csrc/vr_variant.h"
#include "host_scene.h"

using namespace vr;
using namespace hostscene;

namespace {
struct ProbeScene {
    HostScene S;
    SceneParams paired{};      // the views of the kernel compiled for the paired atlas (RendererHIP::fill_params); == S.P when the scene has none
};
int fail(char* err, int errlen, const char* why) {
    if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", why);
    return 1;
}
}  // namespace

extern "C" {

int hp_uniforms_size() { return (int)sizeof(Uniforms); }

// flags: host_scene.h HS_*; 8 = pair the atlases when the product would (vr_variant.h: two grids that can share one, in a scene nothing sends to the run-time variant)
void* hp_scene_create(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                      const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int flags) {
    ProbeScene* ps = new ProbeScene;
    build_scene(ps->S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim, flags);
    SceneParams& P = ps->S.P;
    ps->paired = P;
    if ((flags & 8) && scene_pairs_atlases(P)) {      // (no emission descriptor: a zero emission view, as in host_kernel.cpp build_lane_scene)
        build_paired_atlas(ps->S.dg, ps->S.eg, ps->S.paired);
        ps->paired.density.atlas = ps->S.paired.data();
        ps->paired.emission.atlas = ps->S.paired.data();
        ps->paired.paired = 1;
    }
    return ps;
}
void hp_scene_free(void* h) { delete static_cast<ProbeScene*>(h); }
// out: [0] the map has a compact form, [1] env_div_safe, [2] paired, [3] decoded float atlas present
void hp_scene_info(void* h, int out[4]) {
    const ProbeScene* ps = static_cast<const ProbeScene*>(h);
    out[0] = ps->S.P.env_rgbe != nullptr; out[1] = ps->S.P.env_div_safe; out[2] = ps->paired.paired; out[3] = ps->S.P.density.atlas_f32 != nullptr;
}
// the table arrays themselves, for the tests that change one value on purpose: 0 paired atlas (bytes), 1 warp table (floats), 2 float majorants, 3 fp16 majorants, 4 compact map
void* hp_scene_table(void* h, int which, long long* n) {
    ProbeScene* ps = static_cast<ProbeScene*>(h);
    switch (which) {
    case 0: *n = (long long)ps->S.paired.size(); return ps->S.paired.data();
    case 1: *n = (long long)ps->S.cdf.size(); return ps->S.cdf.data();
    case 2: *n = (long long)ps->S.dg.majorant.size(); return ps->S.dg.majorant.data();
    case 3: *n = (long long)ps->S.dg.majorant16.size(); return ps->S.dg.majorant16.data();
    case 4: *n = (long long)ps->S.rgbe.size(); return ps->S.rgbe.data();
    }
    *n = 0; return nullptr;
}

// 0 ok; 1: the scene cannot serve the form, or a bad item (err says why)
int hp_probe(void* h, int what, int form, const uint32_t* in, float* out, long long n, char* err, int errlen) {
    const ProbeScene* ps = static_cast<const ProbeScene*>(h);
    if (const char* why = probe_form_error(ps->paired, what, form)) return fail(err, errlen, why);
    if (const char* why = probe_items_error(ps->paired, what, form, in, (size_t)n)) return fail(err, errlen, why);
    const SceneParams& P = probe_decode_form(what, form).pair != 0 ? ps->paired : ps->S.P;      // as RendererHIP::probe picks the views
    const int k = probe_out_words(what);
#pragma omp parallel for schedule(static)
    for (long long i = 0; i < n; ++i) probe_item(P, what, form, in + kProbeInWords * i, out + (size_t)k * (size_t)i);
    return 0;
}

// env_pack.h on one texel: returns 1 and the dword, or 0
int hp_pack_texel(const float* rgb, uint32_t* q) { return pack_rgbe_texel(rgb, *q) ? 1 : 0; }
int hp_pack_map(const float* tex, long long n, uint32_t* packed) {
    std::vector<uint32_t> v;
    if (!pack_rgbe_map(tex, (size_t)n, 3, v)) return 0;
    memcpy(packed, v.data(), v.size() * sizeof(uint32_t));
    return 1;
}
// what env_texture makes of one packed texel: the three floats
void hp_unpack_texels(const uint32_t* q, long long n, float* rgb) {
    for (long long i = 0; i < n; ++i) {
        SceneParams P{};
        P.env_rgbe = q + i; P.env_w = 1; P.env_h = 1;
        const v3 c = env_texture(P, 0.5f, 0.5f);
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
    }
}

}  // extern "C"
