// tests/hostkernel/resolve_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The control variate on the expected coverage (volren_amd/csrc/vr_resolve.h) compiled for the host, on the scene host_scene.h builds from the oracle's
// arrays: tests/test_resolve_host.py checks it against a float64 statement of the same definition (tests/hk_resolve.py), and tests/test_gpu_resolve.py
// checks the HIP kernels against it.
#include "host_scene.h"

#include "../../volren_amd/csrc/vr_resolve.h"

using namespace hostscene;

namespace {
struct HostTaps {
    const float* p;        // P, W*H*4
    int32_t at, W;         // the pixel's own index
    void tap(int32_t dx, int32_t dy, float o[4]) const { const float* q = p + 4 * (size_t)(at + dy * W + dx); o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; }
};
}

extern "C" {

// prepare on the scene's frame: fb = W*H*4 -> B, P = W*H*4 each, row 0 at the bottom
void hk_resolve_prepare(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut, const float* env_rgb, int env_w, int env_h,
                        const float* impmap, int imp_dim, int rays, const float* fb, float* B, float* Pq) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    const int W = P.u.resolution[0], H = P.u.resolution[1];
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        resolve_prepare_pixel(fb + 4 * p, resolve_background(P, x, y, rays), B + 4 * p, Pq + 4 * p);
    }
}

// prepare's second half alone, from a B the caller made (synthetic frames): P = W*H*4
void hk_resolve_part(int W, int H, const float* fb, const float* B, float* Pq) {
    for (size_t p = 0; p < (size_t)W * H; ++p) {
        float b[4];
        resolve_prepare_pixel(fb + 4 * p, v3{ B[4 * p], B[4 * p + 1], B[4 * p + 2] }, b, Pq + 4 * p);
    }
}

// resolve: fb, B, P = W*H*4, kappa = W*H (the coverage channel of the features) -> out = W*H*4
void hk_resolve(int W, int H, const float* fb, const float* B, const float* Pq, const float* kappa, float* out) {
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const int32_t p = y * W + x;
        resolve_pixel(HostTaps{ Pq, p, W }, W, H, x, y, fb + 4 * (size_t)p, B + 4 * (size_t)p, kappa[p], out + 4 * (size_t)p);
    }
}

}
