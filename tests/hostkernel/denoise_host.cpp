// tests/hostkernel/denoise_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The a-trous denoiser of the lane code (volren_amd/csrc/vr_denoise.h) compiled for the host: tests/test_denoise_host.py checks it against a
// float64 numpy statement of the filter (tests/hk_denoise.py), and tests/test_gpu_denoise.py checks the HIP kernels against it bit for bit.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../volren_amd/csrc/vr_denoise.h"

using namespace vr;

namespace {
struct HostSrc {
    const float* c;      // W*H*4
    const float* v;      // W*H
    const float* g;      // W*H*8
    void color(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = c[4 * (size_t)i + k]; }
    float var(int32_t i) const { return v[i]; }
    void guide(int32_t i, float o[8]) const { for (int k = 0; k < 8; ++k) o[k] = g[8 * (size_t)i + k]; }
};
DenoiseSigma sigma_of(const float* s) { return DenoiseSigma{ s[0], s[1], s[2], s[3], s[4] }; }
}  // namespace

extern "C" {

// prepare: var = W*H*4 unbiased variances (vr_variance), feat = W*H*8 features -> v (W*H), guide (W*H*8)
void hk_denoise_prepare(int W, int H, int n, const float* var, const float* feat, float* v, float* guide) {
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        v[i] = denoise_mean_variance(var + 4 * i, n);
        denoise_guide(feat + 8 * i, guide + 8 * i);
    }
}

// one iteration of step `step`: (c, v, guide) -> (cout, vout)
void hk_denoise_atrous(int W, int H, int step, const float* c, const float* v, const float* guide, const float* sigma, float* cout, float* vout) {
    const HostSrc src{ c, v, guide };
    const DenoiseSigma sg = sigma_of(sigma);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            denoise_atrous_pixel(src, W, H, x, y, step, sg, cout + 4 * i, vout[i]);
        }
}

// the accepted range of every sigma: out[0] = smallest, out[1] = largest
void hk_denoise_sigma_range(float* out) { out[0] = kDenoiseSigmaMin; out[1] = kDenoiseSigmaMax; }

// the whole filter as RendererHIP::denoise runs it: prepare, then N iterations at steps 1, 2, 4, ... (N = 0: the colour copied)
void hk_denoise(int W, int H, int n, const float* color, const float* var, const float* feat, int N, const float* sigma, float* out) {
    const size_t px = (size_t)W * H;
    std::vector<float> v(px), v2(px), g(8 * px), c(color, color + 4 * px), c2(4 * px);
    hk_denoise_prepare(W, H, n, var, feat, v.data(), g.data());
    for (int k = 0; k < N; ++k) {
        hk_denoise_atrous(W, H, 1 << k, c.data(), v.data(), g.data(), sigma, c2.data(), v2.data());
        c.swap(c2);
        v.swap(v2);
    }
    std::memcpy(out, c.data(), 4 * px * sizeof(float));
}

}
