// tests/hostkernel/demod_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The albedo demodulation of the scattered layer (volren_amd/csrc/vr_demod.h) compiled for the host: the divisor, the split, the variance, the merge and the
// upsampling with demodulated taps.  tests/test_demod_host.py checks them against a float64 statement of the header (tests/hk_demod.py), and
// tests/test_gpu_demod.py checks the HIP kernels' DEMOD instances against them through the public calls.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../volren_amd/csrc/vr_demod.h"

using namespace vr;

namespace {
struct HostTaps {
    const float* L;        // w*h*4
    const float* g;        // w*h*8
    int32_t w;
    void tap(int32_t lx, int32_t ly, float Lq[4], float gq[8]) const {
        const size_t i = (size_t)ly * w + lx;
        for (int c = 0; c < 4; ++c) Lq[c] = L[4 * i + c];
        for (int c = 0; c < 8; ++c) gq[c] = g[8 * i + c];
    }
};
}

extern "C" {

float hk_demod_floor() { return kDemodFloor; }

// feat = n*8 (words 0..3 are read) -> d = n*3
void hk_demod_divisor(int n, const float* feat, float* d) {
    for (size_t p = 0; p < (size_t)n; ++p) demod_divisor(feat + 8 * p, d + 3 * p);
}

// split: y, B = n*4, feat = n*8 -> S = n*4
void hk_demod_split(int n, const float* y, const float* B, const float* feat, float* S) {
    for (size_t p = 0; p < (size_t)n; ++p) demod_split_pixel(y + 4 * p, B + 4 * p, feat + 8 * p, S + 4 * p);
}

// prepare's v: var = n*4 unbiased variances, feat = n*8, counts = n sample counts (one per pixel) -> v = n
void hk_demod_variance(int n, const float* var, const float* feat, const int32_t* counts, float* v) {
    for (size_t p = 0; p < (size_t)n; ++p) v[p] = demod_mean_variance(var + 4 * p, feat + 8 * p, counts[p]);
}

// merge: F, B = n*4, feat = n*8 -> out, L = n*4
void hk_demod_merge(int n, const float* F, const float* B, const float* feat, float* out, float* L) {
    for (size_t p = 0; p < (size_t)n; ++p) demod_merge_pixel(F + 4 * p, B + 4 * p, feat + 8 * p, L + 4 * p, out + 4 * p);
}

// The whole hi frame, as hk_upsample (upsample_host.cpp) takes it.  staged = 0: every tap demodulated as it is read (DemodTaps); 1: the lo layer demodulated
// once per texel into a copy that plain taps read, as the kernel's window holds it
void hk_demod_upsample(int w, int h, int f, int staged, const float* L, const float* glo, const float* ghi, const float* B, const float* sigma, float* out, float* Lout) {
    const DenoiseSigma sg{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] };
    const int W = f * w, H = f * h;
    std::vector<float> copy;
    if (staged) {
        copy.assign(L, L + (size_t)w * h * 4);
        for (size_t q = 0; q < (size_t)w * h; ++q) demod_tap(copy.data() + 4 * q, glo + 8 * q);
    }
    const HostTaps plain{ staged ? copy.data() : L, glo, w };
    const DemodTaps<HostTaps> taps{ plain };
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        if (staged) demod_upsample_pixel(plain, w, h, f, x, y, ghi + 8 * p, B + 4 * p, sg, Lout + 4 * p, out + 4 * p);
        else demod_upsample_pixel(taps, w, h, f, x, y, ghi + 8 * p, B + 4 * p, sg, Lout + 4 * p, out + 4 * p);
    }
}

}
