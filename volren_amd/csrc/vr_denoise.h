// vr_denoise.h -- the edge-avoiding a-trous wavelet filter of the denoiser (host + device lane code).
//
// The spatial part of SVGF (Schied et al. 2017, after Dammertz et al. 2010), guided by the renderer's per-pixel variance and first-scatter
// features (vr_trace.h feature_pixel).  Per-pixel functions only: the HIP kernels (vr_filters.hip denoise_prepare_kernel /
// denoise_atrous_kernel) and the host build of the tests (tests/hostkernel/denoise_host.cpp) run the same code, so the two agree bit for bit.
// The arithmetic is fixed operation by operation (vr_math.h: -ffp-contract=off, IEEE division, the project's exp_ / pow_ / sqrt_ / luma),
// and every sum runs in one order: dy outer, dx inner, from -r to r.  n = the samples behind the framebuffer; row 0 is the bottom row.
//
// Prepare (once per call), pixel p:
//   v_p = (sum_i w_i sqrt(max(var_i, 0)))^2 / n       var = the unbiased per-channel variance (vr_variance), w = luma's weights: the variance of
//                                                      the mean's luminance when the channels are perfectly correlated
//   guide = (albedo.rgb, coverage, g.xyz, depth)       g = normalize(averaged normal), 0 where that normal is 0
// Iteration k = 0..N-1, step s = 2^k, pixel p:
//   vbar_p = the 3x3 Gaussian (1/4, 1/2, 1/4)^2 of v around p (taps outside the frame skipped, weights renormalised)
//   taps q = p + s (dx, dy), dx, dy in -2..2, outside the frame skipped, B3-spline h = (1/16, 1/4, 3/8, 1/4, 1/16):
//   w = h(dx) h(dy) w_c w_k w_n w_d w_a, with
//     w_c = exp(-|L_p - L_q| / (sigma_c sqrt(vbar_p) + 1e-6))                      L = luma of the current colour
//     w_k = exp(-|k_p - k_q| / sigma_k)                                             k = coverage
//     and, only where k_p > 0 and k_q > 0 (1 otherwise):
//     w_n = pow(min(1, max(0, dot(g_p, g_q))), sigma_n)   (1 when either g is 0; exactly 0 for dot <= 0; the float32 dot of two unit
//                                                  vectors can be 1 + 2^-22, and without the clamp w_n > 1 overflows for large sigma_n)
//     w_d = exp(-|d_p - d_q| / (sigma_d max(d_p, d_q) + 1e-6))                     relative depth difference
//     w_a = exp(-|a_p - a_q|^2 / sigma_a^2)
//   The centre tap's edge-stopping factors are 1 by definition: its weight is exactly (3/8)^2 > 0.
//   c'_p = sum w c_q / sum w (all four channels, the same weights), v'_p = sum w^2 v_q / (sum w)^2.
// N = 0 returns the colour bit for bit.  No albedo demodulation.  The temporal half of SVGF is vr_temporal.h, with vr_moments.h
// for its variance estimate: it runs in front of these iterations.
//
// Every sigma lies in [2^-60, 2^60] (vr_set_float "denoise_sigma" refuses the rest): sigma_a^2 stays a normal float, so two equal albedos give
// 0 / sigma_a^2 = 0 and not 0 / 0, and a device that flushes subnormals computes what the host does.
// Defaults: N = 5, (sigma_c, sigma_n, sigma_d, sigma_k, sigma_a) = (4, 0.5, 0.1, 0.25, 0.2), chosen from a sweep of 80 settings (DESIGN.md 5
// "Denoiser": relative L2 to a 1024-spp frame on c2 / c3 / c4 at 256^2, 16 and 64 spp).  The averaged first-scatter normals of a volume are
// noisy, so a sharp normal weight (sigma_n = 16, the starting point) stops the filter on c2 / c3: 0.66 / 0.65 of the raw error at 16 spp,
// against 0.33 / 0.39 with 0.5.
#pragma once

#include "vr_math.h"

namespace vr {

struct DenoiseSigma { float c, n, d, k, a; };          // colour, normal, depth, coverage, albedo: the order of vr_set_float "denoise_sigma"
constexpr int32_t kDenoiseDefaultIterations = 5;
constexpr int32_t kDenoiseMaxIterations = 10;
constexpr float kDenoiseDefaultSigma[5] = { 4.0f, 0.5f, 0.1f, 0.25f, 0.2f };
constexpr float kDenoiseSigmaMin = 0x1p-60f, kDenoiseSigmaMax = 0x1p60f;      // the accepted range of every sigma

// variance of the mean's luminance from the unbiased per-channel variance of n >= 1 samples
VR_HD float denoise_mean_variance(const float var[4], int32_t n) {
    const float s = luma(v3{ sqrt_(max_(var[0], 0.0f)), sqrt_(max_(var[1], 0.0f)), sqrt_(max_(var[2], 0.0f)) });
    return (s * s) / (float)n;
}

// the guide of one pixel from its features (albedo.rgb, coverage, normal.xyz, depth): the same layout with the normal normalised
VR_HD void denoise_guide(const float feat[8], float g[8]) {
    for (int32_t i = 0; i < 4; ++i) g[i] = feat[i];
    const v3 n = v3{ feat[4], feat[5], feat[6] };
    const float nn = dot(n, n);
    const v3 u = nn > 0.0f ? n * (1.0f / sqrt_(nn)) : v3{ 0.0f, 0.0f, 0.0f };
    g[4] = u.x; g[5] = u.y; g[6] = u.z;
    g[7] = feat[7];
}

// One a-trous iteration at pixel (px, py) of a W x H frame, step `step`.  Src reads the iteration's inputs by pixel index y * W + x:
//   void color(int32_t i, float c[4]) const;   float var(int32_t i) const;   void guide(int32_t i, float g[8]) const;
template <class Src>
VR_HD void denoise_atrous_pixel(const Src& src, int32_t W, int32_t H, int32_t px, int32_t py, int32_t step, const DenoiseSigma& sg,
                                float out[4], float& vout) {
    const float g3[3] = { 0.25f, 0.5f, 0.25f };
    const float b3[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
    float vs = 0.0f, gs = 0.0f;
    for (int32_t dy = -1; dy <= 1; ++dy) {
        const int32_t y = py + dy;
        if (y < 0 || y >= H) continue;
        for (int32_t dx = -1; dx <= 1; ++dx) {
            const int32_t x = px + dx;
            if (x < 0 || x >= W) continue;
            const float w = g3[dx + 1] * g3[dy + 1];
            vs = vs + w * src.var(y * W + x);
            gs = gs + w;
        }
    }
    const float vbar = vs / gs;
    const int32_t ip = py * W + px;
    float cp[4], gp[8];
    src.color(ip, cp);
    src.guide(ip, gp);
    const float Lp = luma(v3{ cp[0], cp[1], cp[2] });
    const float dc = sg.c * sqrt_(vbar) + 1e-6f;
    const float sa2 = sg.a * sg.a;
    const v3 np = v3{ gp[4], gp[5], gp[6] }, ap = v3{ gp[0], gp[1], gp[2] };
    const bool np0 = np.x == 0.0f && np.y == 0.0f && np.z == 0.0f;
    float acc[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    float sw = 0.0f, sv = 0.0f;
    for (int32_t dy = -2; dy <= 2; ++dy) {
        const int32_t y = py + step * dy;
        if (y < 0 || y >= H) continue;
        for (int32_t dx = -2; dx <= 2; ++dx) {
            const int32_t x = px + step * dx;
            if (x < 0 || x >= W) continue;
            const int32_t iq = y * W + x;
            float cq[4];
            src.color(iq, cq);
            const float vq = src.var(iq);
            float w = b3[dx + 2] * b3[dy + 2];
            if (dx != 0 || dy != 0) {
                float gq[8];
                src.guide(iq, gq);
                const float Lq = luma(v3{ cq[0], cq[1], cq[2] });
                w = w * exp_(-abs_(Lp - Lq) / dc);
                w = w * exp_(-abs_(gp[3] - gq[3]) / sg.k);
                if (gp[3] > 0.0f && gq[3] > 0.0f) {
                    const v3 nq = v3{ gq[4], gq[5], gq[6] }, da = ap - v3{ gq[0], gq[1], gq[2] };
                    const bool nq0 = nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f;
                    const float wn = (np0 || nq0) ? 1.0f : pow_(min_(1.0f, max_(0.0f, dot(np, nq))), sg.n);
                    const float wd = exp_(-abs_(gp[7] - gq[7]) / (sg.d * max_(gp[7], gq[7]) + 1e-6f));
                    const float wa = exp_(-dot(da, da) / sa2);
                    w = w * wn;
                    w = w * wd;
                    w = w * wa;
                }
            }
            for (int32_t c = 0; c < 4; ++c) acc[c] = acc[c] + w * cq[c];
            sw = sw + w;
            sv = sv + (w * w) * vq;
        }
    }
    for (int32_t c = 0; c < 4; ++c) out[c] = acc[c] / sw;
    vout = sv / (sw * sw);
}

}  // namespace vr
