// tests/hostkernel/sky_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The clear-tile classifier (volren_amd/csrc/vr_sky_tiles.h) and the primary-miss sample (vr_trace.h sky_sample) compiled for the host:
// tests/test_sky_tiles_host.py holds the classifier to a lattice of slab tests and to the oracle, and sky_sample to the oracle's trace_pixel_sample bit for bit.
#include <cstdint>
#include <vector>

#include "host_scene.h"
#include "../../volren_amd/csrc/vr_sky_tiles.h"

using namespace vr;

namespace {
// the uniforms as a launch hands them to the classifier: cam_z as RendererHIP::fill_params / host_scene.h form it
SceneParams params_of(const Uniforms* u) {
    SceneParams P{};
    P.u = *u;
    P.cam_z = -0.5f / tan_(0.5f * kPi * u->cam_fov / 180.f);
    return P;
}
}  // namespace

extern "C" {

int hk_sky_uniforms_size(void) { return (int)sizeof(Uniforms); }

// clear[i] = 1 when tile tiles[i] of the frame u->resolution is clear
void hk_sky_classify(const Uniforms* u, const int32_t* tiles, int n, uint8_t* clear) { sky_classify_tiles(params_of(u), tiles, n, clear); }

// the split of a list (n_ids == 0: the whole frame's n_tiles tiles): march tiles, then clear tiles, into out; returns the number of clear ones
int hk_sky_split(const Uniforms* u, const int32_t* ids, int n_ids, int n_tiles, int32_t* out) {
    std::vector<int32_t> march, sky;
    sky_split_tiles(params_of(u), std::vector<int32_t>(ids, ids + n_ids), n_tiles, march, sky);
    size_t k = 0;
    for (int32_t t : march) out[k++] = t;
    for (int32_t t : sky) out[k++] = t;
    return (int)sky.size();
}

// sky_sample of n (px, py, sample number) triples with hashed seeds: out[4 i ..] the sample, miss[i] = what sky_sample returned
void hk_sky_samples(const Uniforms* u, const hostscene::hk_grid_desc* density, const float* lut, const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim,
                    const int32_t* items, int n, float* out, int32_t* miss) {
    hostscene::HostScene S;
    hostscene::build_scene(S, u, density, nullptr, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    for (int i = 0; i < n; ++i) {
        const int32_t px = items[3 * i], py = items[3 * i + 1], smp = items[3 * i + 2];
        float L[4] = { -1.0f, -1.0f, -1.0f, -1.0f };
        miss[i] = sky_sample(P, px, py, path_seed((uint32_t)P.u.seed, P.u.resolution[0], px, py, smp), L) ? 1 : 0;
        for (int c = 0; c < 4; ++c) out[4 * i + c] = L[c];
    }
}

}
