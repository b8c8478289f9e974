// tests/hostkernel/regress_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The one-pass local-regression filter (volren_amd/csrc/vr_regress.h) compiled for the host: tests/test_regress_host.py checks it against a float64
// statement of the same definition (tests/hk_regress.py), and tests/test_gpu_regress.py checks the HIP kernel against it.
#include <stddef.h>
#include <stdint.h>

#include "../../volren_amd/csrc/vr_regress.h"

using namespace vr;

namespace {
struct HostSrc {
    const float* S;      // W*H*4
    const float* g;      // W*H*8
    int32_t W, px, py;
    void tap(int32_t dx, int32_t dy, float s[4], float o[8]) const {
        const size_t i = (size_t)(py + dy) * W + (px + dx);
        for (int k = 0; k < 4; ++k) s[k] = S[4 * i + k];
        for (int k = 0; k < 8; ++k) o[k] = g[8 * i + k];
    }
};
}  // namespace

extern "C" {

// the filter on a whole frame: S = W*H*4, guide = W*H*8 (hk_denoise_prepare's), sigma = 5 -> F = W*H*4
void hk_regress(int W, int H, const float* S, const float* guide, const float* sigma, float ridge, float* F) {
    const DenoiseSigma sg{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) regress_pixel(HostSrc{ S, guide, W, x, y }, W, H, x, y, sg, ridge, F + 4 * ((size_t)y * W + x));
}

// beta_0 of one system: A = 8 x 8 row-major (the upper triangle is read), b = 8 x 3 -> Ct = 3; both inputs are left as they were
void hk_regress_solve(const float* A, const float* b, float floor, float* Ct) {
    float a[kRegressTerms][kRegressTerms], r[kRegressTerms][3];
    for (int i = 0; i < kRegressTerms; ++i) {
        for (int j = 0; j < kRegressTerms; ++j) a[i][j] = A[kRegressTerms * i + j];
        for (int c = 0; c < 3; ++c) r[i][c] = b[3 * i + c];
    }
    regress_solve(a, r, floor, Ct);
}

// the filter once more, with the header's own counter: dropped = W*H, how many columns regress_solve dropped at each pixel, -1 where the pixel never reaches the
// solve (kappa_p = 0, A_00 at or below the smallest weight, or ridge 0)
void hk_regress_dropped(int W, int H, const float* S, const float* guide, const float* sigma, float ridge, float* F, int32_t* dropped) {
    const DenoiseSigma sg{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            regress_pixel(HostSrc{ S, guide, W, x, y }, W, H, x, y, sg, ridge, F + 4 * i, dropped + i);
        }
}

// (radius, terms, smallest weight, smallest depth, pivot floor, smallest ridge, largest ridge, default ridge)
void hk_regress_constants(float* out) {
    out[0] = (float)kRegressRadius; out[1] = (float)kRegressTerms; out[2] = kRegressMinWeight; out[3] = kRegressMinDepth; out[4] = kRegressPivotFloor;
    out[5] = kRegressRidgeMin; out[6] = kRegressRidgeMax; out[7] = kRegressDefaultRidge;
}

int hk_regress_ridge_ok(float v) { return regress_ridge_ok(v) ? 1 : 0; }

}
