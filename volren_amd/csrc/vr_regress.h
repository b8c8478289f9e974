// vr_regress.h -- the one-pass local-regression filter of the scattered layer (host + device lane code).
//
// With "denoise_layers" = 1 the only noisy quantity the denoiser sees is C, the conditional mean of the scattered light (vr_layers.h: a pixel shows
// (1 - kappa) B + kappa C), and its guide -- coverage, depth, normal, albedo from the expected-value pass (vr_expected.h) -- carries no noise at all.  The a-trous
// iterations of vr_denoise.h were built for a noisy guide: five zero-order passes, a colour weight driven by the frame's sample variance, a footprint of +-62
// pixels.  With "denoise_filter" = 1 ONE pass over an 11 x 11 window takes their place: a weighted least-squares fit of C, per pixel, as an affine function of
// the guide, evaluated at the pixel itself.  No colour weight, no variance: the pass neither reads nor writes v.  Resolve, split, the temporal blend,
// rejection, moments and the merge stay as they are.
// Per-pixel functions only: the HIP kernel (vr_filters.hip denoise_regress_kernel) and the host build of the tests (tests/hostkernel/regress_host.cpp) run the
// same code, so the two agree bit for bit.  The arithmetic is float32, fixed operation by operation (vr_math.h: -ffp-contract=off, IEEE division, exp_ / pow_,
// max_); a * b + c below is two roundings, every sum starts from +0 and runs in one order.  Frames are W x H texels, row 0 at the bottom.
//
// Inputs at pixel p: S_p, what the a-trous would read -- layers_split's S, under vr_denoise_temporal the blended history colour: rgb signed, premultiplied by
// the coverage S_p.a -- and g_p = (albedo.rgb, kappa, unit normal.xyz, depth), vr_denoise.h's guide.  Without the temporal pass S_p.a is kappa_p bit for bit.
// sigma = the renderer's "denoise_sigma" (its colour and coverage entries are not used), lambda = "denoise_ridge".
//
// kappa_p == 0:  F_p = (0, 0, 0, 0) and nothing else is read.  Otherwise
//   rd  = 1 / max_(d_p, 2^-20)                                                      one division per pixel
//   taps q = p + (dx, dy), dy = -5..5 outer, dx = -5..5 inner; a tap outside the frame is skipped before anything is read; a tap counts only where
//   S_q.a > 2^-20 and kappa_q > 0 (a NaN in either: it does not count) -- the centre is a tap like the others.
//   u   = s(dx) * s(dy),  s(d) = exp(-d^2 / (2 * 2.5^2)) tabulated as 11 float32 constants (regress_pixel's s[])
//   e   = 1 at the centre, else w_n * w_d * w_a of vr_denoise.h between g_p and g_q, multiplied in its order from 1 (vr_upsample.h upsample_edge)
//   se  = u * e;   w = se * S_q.a                                                   the weight of the tap's target c_q = S_q.rgb / S_q.a
//   t   = se * S_q.rgb                                                              = w c_q without the division: this product IS the definition
//   x   = (1,  (d_q - d_p) * rd,  n_q - n_p (3),  a_q - a_p (3))                    eight regressors, x_0 the intercept
//   A_0j += w x_j (A_00 += w);  A_ij += (w x_i) * x_j for 1 <= i <= j <= 7;  b_ic += x_i * t_c (b_0c += t_c)        36 + 24 sums
// A_00 <= 2^-20:  no covered tap, F_p = (0, 0, 0, kappa_p).  Otherwise
//   lambda == 0:  Ct = b_0 / A_00                                                   zero order: the normalised weighted mean, no solve
//   lambda > 0:   rl = lambda * A_00;  A_ii = A_ii + rl for i = 1..7;  floor = 2^-20 * rl; then the LDL^T elimination of regress_solve in the order 0, 1, .. 7:
//     a_k = A_kk as it stands before the elimination (ridge included), k = 1..7
//     pivot k: d_k = A_kk; column k is KEPT if k == 0 or (d_k > floor and d_k > 2^-12 a_k) (a NaN pivot: dropped); r_k = 1 / d_k;
//       for i = k+1..7: l = kept ? A_ki * r_k : 0;  A_ij = A_ij - l * A_kj for j = i..7;  b_ic = b_ic - l * b_kc;  then A_ki = l
//     back, k = 7..0: beta_kc = kept ? (b_kc * r_k - A_k,k+1 * beta_k+1,c - ... - A_k7 * beta_7c, subtracted in that order) : 0
//     Ct = beta_0.  In exact arithmetic every pivot after the first is >= rl (a sum of squares plus the ridge), so the floor drops only a column that rounding
//     emptied.  The second test is about a column that rounding did NOT empty but left meaningless: d_k is what remains of a_k after up to seven subtractions,
//     known to some ten 2^-24 a_k (a_k is a sum over up to 121 taps) and no better, and a kept column moves Ct by about that times a_k / d_k of the
//     window mean -- a regressor that sits far from 0
//     over the whole window and hardly varies in it (depth 0 at the pixel, so rd = 2^20, over a flat neighbourhood) once gave pivots of either sign and of any size
//     above the floor, and a Ct off by more than the layer's whole range.  A column that keeps less than 2^-12 of its own diagonal is therefore dropped as well: a
//     kept column then costs at most some ten 2^-12 relative.  With regressors of size s the share is at least lambda / (s^2 + lambda): for unit normals, albedos
//     and relative depths, s <= 2, a lambda >= 2^-10 keeps every pivot above the test by the ridge alone, and the test changes nothing.  A dropped column's coefficient is 0 and the others are fitted without it.
//   F_p.rgb = kappa_p * Ct;   F_p.a = kappa_p
// The unchanged merge (vr_layers.h) then has F.a = kappa_p: its ratio is kappa_p / kappa_p = 1 where kappa_p > 2^-20 and not taken below, so L.rgb = F.rgb and
// out = max_(G + L.rgb, 0).  EVERY pixel with kappa_p = 0 comes out as B bit for bit, next to the volume and far from it: F = 0, G = 1 * B, B >= 0.  (The
// a-trous leaves such a pixel the filtered frame where its footprint met no coverage.)  Nothing is sanitised: a NaN in S.rgb of a tap that counts, or in the
// guide of the pixel or of such a tap, makes F_p NaN -- and only the pixels whose window holds it.
//
// Why first order, and why not by default.  A zero-order estimate cannot follow a gradient of C, and the guide describes C's gradients without noise; the ridge
// lambda A_00 on the seven slopes keeps the fit from spending a thin, noisy window's few degrees of freedom on them.  Measured, the slopes pay on
// the dense grid from 16 spp on and cost on thin smoke at 2 and 4 spp, and no lambda > 0 of the sweep beats lambda = 0 on the mean: the default is zero order.
// What it inherits: everything vr_layers.h does.
#pragma once

#include "vr_denoise.h"
#include "vr_math.h"
#include "vr_upsample.h"

namespace vr {

constexpr int32_t kRegressRadius = 5;                  // the window is 11 x 11
constexpr int32_t kRegressTerms = 8;                   // the intercept, depth, normal (3), albedo (3)
constexpr float kRegressMinWeight = 0x1p-20f;          // the smallest coverage of a tap that counts, and the smallest A_00 the pixel divides by
constexpr float kRegressMinDepth = 0x1p-20f;           // the smallest depth the depth regressor is scaled by
constexpr float kRegressPivotFloor = 0x1p-20f;         // a pivot not above this times lambda A_00 drops its column
constexpr float kRegressPivotShare = 0x1p-12f;         // ... and so does one not above this times the column's own diagonal before the elimination
constexpr float kRegressRidgeMin = 0x1p-20f, kRegressRidgeMax = 0x1p20f;      // the accepted range of "denoise_ridge" besides 0
// zero order: in the sweep of {0, 0.01, 0.1, 1, 10} over five scenes at 2..64 spp no lambda > 0 beats it on the mean (tests/test_regress_host.py)
constexpr float kRegressDefaultRidge = 0.0f;

VR_HD bool regress_ridge_ok(float v) { return v == 0.0f || (v >= kRegressRidgeMin && v <= kRegressRidgeMax); }

// beta_0 of the ridged normal equations: A the upper triangle (A[i][j], i <= j; the rest is not read), b the right-hand sides, both destroyed.
// dropped (tests): receives the number of columns that were not kept
VR_HD void regress_solve(float A[kRegressTerms][kRegressTerms], float b[kRegressTerms][3], float floor, float Ct[3], int32_t* dropped = nullptr) {
    constexpr int32_t n = kRegressTerms;
    bool kept[n];
    float r[n], share[n];
#pragma unroll
    for (int32_t k = 0; k < n; ++k) share[k] = kRegressPivotShare * A[k][k];
#pragma unroll
    for (int32_t k = 0; k < n; ++k) {
        const float d = A[k][k];
        kept[k] = k == 0 || (d > floor && d > share[k]);
        r[k] = 1.0f / d;
#pragma unroll
        for (int32_t i = k + 1; i < n; ++i) {
            const float l = kept[k] ? A[k][i] * r[k] : 0.0f;
#pragma unroll
            for (int32_t j = i; j < n; ++j) A[i][j] = A[i][j] - l * A[k][j];
#pragma unroll
            for (int32_t c = 0; c < 3; ++c) b[i][c] = b[i][c] - l * b[k][c];
            A[k][i] = l;
        }
    }
    float beta[n][3];
#pragma unroll
    for (int32_t k = n - 1; k >= 0; --k) {
#pragma unroll
        for (int32_t c = 0; c < 3; ++c) {
            float v = b[k][c] * r[k];
#pragma unroll
            for (int32_t i = k + 1; i < n; ++i) v = v - A[k][i] * beta[i][c];
            beta[k][c] = kept[k] ? v : 0.0f;
        }
    }
    for (int32_t c = 0; c < 3; ++c) Ct[c] = beta[0][c];
    if (dropped) {
        *dropped = 0;
        for (int32_t k = 0; k < n; ++k) *dropped += kept[k] ? 0 : 1;
    }
}

// The filter at pixel (px, py) of a W x H frame.  Src answers, for (px + dx, py + dy) inside the frame only, |dx|, |dy| <= kRegressRadius,
//   void tap(int32_t dx, int32_t dy, float S[4], float g[8]) const      the texel of S and the guide there
// -> F, what the merge reads.  dropped (tests): receives the number of columns regress_solve dropped, -1 where the pixel never reaches it.
template <class Src>
VR_HD void regress_pixel(const Src& src, int32_t W, int32_t H, int32_t px, int32_t py, const DenoiseSigma& sg, float ridge, float F[4], int32_t* dropped = nullptr) {
    constexpr int32_t n = kRegressTerms, R = kRegressRadius;
    // s(d) = exp(-d^2 / 12.5), d = -5..5, rounded to float32
    const float s[2 * R + 1] = { 0.135335283f, 0.278037300f, 0.486752256f, 0.726149037f, 0.923116346f, 1.0f, 0.923116346f, 0.726149037f, 0.486752256f, 0.278037300f, 0.135335283f };
    float Sp[4], gp[8];
    src.tap(0, 0, Sp, gp);
    const float kp = gp[3];
    F[0] = 0.0f; F[1] = 0.0f; F[2] = 0.0f; F[3] = kp;
    if (dropped) *dropped = -1;
    if (kp == 0.0f) { F[3] = 0.0f; return; }
    const float rd = 1.0f / max_(gp[7], kRegressMinDepth);
    float A[n][n], b[n][3];
#pragma unroll
    for (int32_t i = 0; i < n; ++i) {
#pragma unroll
        for (int32_t j = 0; j < n; ++j) A[i][j] = 0.0f;
        b[i][0] = 0.0f; b[i][1] = 0.0f; b[i][2] = 0.0f;
    }
    for (int32_t dy = -R; dy <= R; ++dy) {
        const int32_t y = py + dy;
        if (y < 0 || y >= H) continue;
        for (int32_t dx = -R; dx <= R; ++dx) {
            const int32_t x = px + dx;
            if (x < 0 || x >= W) continue;
            float Sq[4], gq[8];
            src.tap(dx, dy, Sq, gq);
            if (!(Sq[3] > kRegressMinWeight && gq[3] > 0.0f)) continue;
            const float u = s[dx + R] * s[dy + R];
            const float e = (dx != 0 || dy != 0) ? upsample_edge(gp, gq, sg) : 1.0f;
            const float se = u * e;
            const float w = se * Sq[3];
            const float t[3] = { se * Sq[0], se * Sq[1], se * Sq[2] };
            const float xq[n] = { 1.0f, (gq[7] - gp[7]) * rd, gq[4] - gp[4], gq[5] - gp[5], gq[6] - gp[6], gq[0] - gp[0], gq[1] - gp[1], gq[2] - gp[2] };
            A[0][0] = A[0][0] + w;
            b[0][0] = b[0][0] + t[0]; b[0][1] = b[0][1] + t[1]; b[0][2] = b[0][2] + t[2];
#pragma unroll
            for (int32_t i = 1; i < n; ++i) {
                const float wx = w * xq[i];
                A[0][i] = A[0][i] + wx;
#pragma unroll
                for (int32_t j = i; j < n; ++j) A[i][j] = A[i][j] + wx * xq[j];
#pragma unroll
                for (int32_t c = 0; c < 3; ++c) b[i][c] = b[i][c] + xq[i] * t[c];
            }
        }
    }
    if (A[0][0] <= kRegressMinWeight) return;
    float Ct[3];
    if (ridge == 0.0f) {
        Ct[0] = b[0][0] / A[0][0]; Ct[1] = b[0][1] / A[0][0]; Ct[2] = b[0][2] / A[0][0];
    } else {
        const float rl = ridge * A[0][0];
#pragma unroll
        for (int32_t i = 1; i < n; ++i) A[i][i] = A[i][i] + rl;
        regress_solve(A, b, kRegressPivotFloor * rl, Ct, dropped);
    }
    F[0] = kp * Ct[0]; F[1] = kp * Ct[1]; F[2] = kp * Ct[2];
}

}  // namespace vr
