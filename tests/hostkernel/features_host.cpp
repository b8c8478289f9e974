// tests/hostkernel/features_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The denoiser feature pass of the lane code (volren_amd/csrc/vr_trace.h feature_sample / feature_pixel) compiled for the host, on the scene
// host_kernel.cpp builds from the oracle's arrays: tests/test_features_host.py checks it against the oracle's orc_sample_volume, and
// tests/test_gpu_features.py checks the HIP kernel against it.
#include "host_kernel.cpp"

extern "C" {

// every (pixel, sample) of a W x H frame, samples 1..spp: hit[(y * W + x) * spp + s - 1] = feature_sample's result (0 miss, 1 hit, 2 lost),
// out[7 per entry] = t, albedo.rgb, normal.xyz (untouched unless hit = 1)
void hk_feature_sample(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                       const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int spp, int32_t* hit, float* out) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    const int W = P.u.resolution[0], H = P.u.resolution[1];
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) for (int s = 1; s <= spp; ++s) {
        const size_t i = ((size_t)y * W + x) * (size_t)spp + (size_t)(s - 1);
        float t = 0.0f;
        v3 a{ 0, 0, 0 }, n{ 0, 0, 0 };
        const int32_t r = P.u.use_tf ? feature_sample<true>(P, x, y, s, t, a, n) : feature_sample<false>(P, x, y, s, t, a, n);
        hit[i] = r;
        if (r != FEAT_HIT) continue;
        float* o = out + 7 * i;
        o[0] = t; o[1] = a.x; o[2] = a.y; o[3] = a.z; o[4] = n.x; o[5] = n.y; o[6] = n.z;
    }
}

// the per-pixel pass: out = W*H*8 floats, (albedo.rgb, coverage, normal.xyz, depth), row 0 at the bottom; returns the pixels that lost a sample
int hk_feature_pass(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                     const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int spp, float* out) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    const int W = P.u.resolution[0], H = P.u.resolution[1];
    int lost = 0;
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        float* o = out + 8 * ((size_t)y * W + x);
        lost += (P.u.use_tf ? feature_pixel<true>(P, x, y, spp, o) : feature_pixel<false>(P, x, y, spp, o)) ? 0 : 1;
    }
    return lost;
}

}
