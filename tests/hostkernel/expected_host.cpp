// tests/hostkernel/expected_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The expected-value feature pass (volren_amd/csrc/vr_expected.h expected_pixel) compiled for the host, on the scene host_scene.h builds from the
// oracle's arrays: tests/test_expected_host.py checks it against a float64 statement of the same definition (tests/hk_expected.py), and
// tests/test_gpu_expected.py checks the HIP kernel against it.
#include "host_scene.h"

#include "../../volren_amd/csrc/vr_expected.h"

using namespace hostscene;

extern "C" {

// the per-pixel pass: out = W*H*8 floats, (albedo.rgb, coverage, normal.xyz, depth), row 0 at the bottom.  info (may be null): per pixel rays * rays
// entries of 3 int32 (sub-ray j * rays + i): its step count m (0: it contributed nothing), the steps it ran, and the bits of the transmittance it ended with
void hk_expected_pass(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                      const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int rays, float* out, int32_t* info) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    const int W = P.u.resolution[0], H = P.u.resolution[1];
    ExpectedRayInfo ri[16];
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        float* o = out + 8 * p;
        if (!info) {
            if (P.u.use_tf) expected_pixel<true>(P, x, y, rays, o); else expected_pixel<false>(P, x, y, rays, o);
            continue;
        }
        if (P.u.use_tf) expected_pixel<true, true>(P, x, y, rays, o, ri); else expected_pixel<false, true>(P, x, y, rays, o, ri);
        for (int k = 0; k < rays * rays; ++k) {
            int32_t* d = info + 3 * (p * (size_t)(rays * rays) + (size_t)k);
            d[0] = ri[k].m; d[1] = ri[k].steps; d[2] = (int32_t)f2u(ri[k].T);
        }
    }
}

}
