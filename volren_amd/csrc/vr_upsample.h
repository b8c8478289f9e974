// vr_upsample.h -- the denoised scattered layer of a small frame rebuilt at f times the size under a full-resolution guide (host + device lane code).
//
// A pixel shows (1 - kappa) B + kappa C (vr_layers.h).  kappa and B are functions of the camera ray alone: the expected-value pass (vr_expected.h) and
// vr_resolve.h's background evaluate them at any resolution without one path-tracing sample, and everything sharp in a smoke frame -- the silhouette ramp, the
// sky's texture through thin smoke -- lives in them.  C is smooth after the filter.  So C is path-traced and filtered on a frame f times smaller per axis (the same
// samples buy f^2 times the spp per pixel there, and a better variance for the filter), and the full-size picture is rebuilt from it under a guide of the full size.
// Per-pixel functions only: the HIP kernel (vr_filters.hip upsample_kernel) and the host build of the tests (tests/hostkernel/upsample_host.cpp) run the same
// code, so the two agree bit for bit.  The arithmetic is fixed operation by operation (vr_math.h: -ffp-contract=off, IEEE division, exp_ / pow_, max_); a * b + c
// below is two roundings, and every sum runs in one order.  Frames have row 0 at the bottom.
//
// "lo" is the renderer's frame, w x h; f in 2..4; "hi" is the output, W = f w by H = f h.
// Lo inputs, pixel q: L_q, the layer of vr_layers.h's merge (rgb premultiplied by the exact kappa_q, alpha = kappa_q), and g_q, vr_denoise.h's guide of the lo
// feature buffer.  Hi inputs, pixel p: the feature buffer of an expected-value pass at W x H (kappa_p its coverage word, g_p its guide), and B_p =
// resolve_background(P_hi, px, py, rays), 0 with the environment hidden.
// At hi pixel (x, y), per axis (x shown):
//   2x + 1 - f = 2f x0 + r, x0 the floor quotient, 0 <= r < 2f;   a = float(r) / float(2f)      (the numerator is exact: one rounding)
//   x0 is the lo pixel whose centre lies at or below the hi pixel's centre, a the fraction of a lo pixel between the two.  At f = 2, a is 0.25 or 0.75.
//   b_0(a) = (1 - a)^3 / 6,  b_1(a) = (3 a^3 - 6 a^2 + 4) / 6,  b_2(a) = (-3 a^3 + 3 a^2 + 3 a + 1) / 6,  b_3(a) = a^3 / 6      the uniform cubic B-spline:
//   never negative, a partition of unity, C2 -- no overshoot on a premultiplied layer, no lattice of the lo frame in the hi one (upsample_spline spells the operations out)
// Taps q = (x0 - 1 + i, y0 - 1 + j), j = 0..3 outer, i = 0..3 inner; a tap outside the lo frame is skipped before anything is read.
//   s = b_i(a_x) * b_j(a_y)
//   e = w_n * w_d * w_a, vr_denoise.h's normal, depth and albedo weights between g_p and g_q with the renderer's "denoise_sigma", under that header's rule: only
//       where kappa_p > 0 and kappa_q > 0, 1 otherwise.  No colour weight: there is no hi colour.  No coverage weight either (DESIGN.md 5 has the measurement:
//       kappa_p is put back exactly below, and a weight on |kappa_p - kappa_q| only starves the ramp's pixels of taps).
//   four sums from 0 in tap order:  N_e += (s e) L_q.rgb;  D_e += (s e) kappa_q;  N_s += s L_q.rgb;  D_s += s kappa_q
// C = N_e / D_e where D_e > 2^-20, else N_s / D_s where D_s > 2^-20, else 0: the ratio of premultiplied sums is the merge's normalisation again (vr_layers.h) --
// it interpolates the conditional mean C -- with the plain spline as the tier for a pixel whose guide stops every tap, and nothing where no tap is covered.
//   L_p.rgb = kappa_p * C;   L_p.a = kappa_p                    the exact hi ramp put back
//   out.rgb = max_(G_p + L_p.rgb, 0), G_p = layers_background(B_p, kappa_p);   out.a = kappa_p
// A hi pixel with kappa_p = 0 comes out as B_p bit for bit (finite C: 0 * C = +-0, G = 1 * B, B >= 0).  Nothing is sanitised: a NaN in a tap that counts makes
// the pixel NaN.
//
// What it inherits: everything vr_layers.h does (the march's coverage bias without a transfer function, the refusals of resolve()), and the camera and scene of
// the denoise call -- the hi guide is marched when the call is made, so they are the caller's to keep as they were.
#pragma once

#include "vr_denoise.h"
#include "vr_layers.h"
#include "vr_math.h"

namespace vr {

constexpr int32_t kUpsampleMinFactor = 2, kUpsampleMaxFactor = 4;
constexpr float kUpsampleMinWeight = 0x1p-20f;         // the smallest sum of weighted coverage either tier divides by

// per axis: hi coordinate x of a frame f times the lo one -> the lo pixel x0 at or below its centre (-1 for the first hi pixels) and the numerator r of the
// fraction, 2x + 1 - f = 2f x0 + r.  The quotient is taken of a numerator moved up by 2f, which is positive: the floor, not C's truncation
VR_HD void upsample_split(int32_t x, int32_t f, int32_t& x0, int32_t& r) {
    const int32_t n = 2 * x + 1 + f;
    x0 = n / (2 * f) - 1;
    r = n - 2 * f * (x0 + 1);
}

// the four weights of the uniform cubic B-spline at fraction a in [0, 1)
VR_HD void upsample_spline(float a, float b[4]) {
    const float a2 = a * a, a3 = a2 * a, oma = 1.0f - a;
    b[0] = ((oma * oma) * oma) / 6.0f;
    b[1] = ((3.0f * a3 - 6.0f * a2) + 4.0f) / 6.0f;
    b[2] = (((-3.0f * a3 + 3.0f * a2) + 3.0f * a) + 1.0f) / 6.0f;
    b[3] = a3 / 6.0f;
}

// e between two guides: the expressions of denoise_atrous_pixel's normal, depth and albedo weights, multiplied in its order from 1
VR_HD float upsample_edge(const float gp[8], const float gq[8], const DenoiseSigma& sg) {
    if (!(gp[3] > 0.0f && gq[3] > 0.0f)) return 1.0f;
    const v3 np = v3{ gp[4], gp[5], gp[6] }, nq = v3{ gq[4], gq[5], gq[6] }, da = v3{ gp[0], gp[1], gp[2] } - v3{ gq[0], gq[1], gq[2] };
    const bool np0 = np.x == 0.0f && np.y == 0.0f && np.z == 0.0f, nq0 = nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f;
    const float wn = (np0 || nq0) ? 1.0f : pow_(min_(1.0f, max_(0.0f, dot(np, nq))), sg.n);
    const float wd = exp_(-abs_(gp[7] - gq[7]) / (sg.d * max_(gp[7], gq[7]) + 1e-6f));
    const float wa = exp_(-dot(da, da) / (sg.a * sg.a));
    float e = 1.0f * wn;
    e = e * wd;
    e = e * wa;
    return e;
}

// Hi pixel (x, y) of a frame f times the w x h lo frame: gp its guide, B its background.  Src answers, for lo pixels inside the lo frame only,
//   void tap(int32_t lx, int32_t ly, float L[4], float g[8]) const      the layer's texel and the guide of lo pixel (lx, ly)
// -> L the hi layer, out the hi frame.
template <class Src>
VR_HD void upsample_pixel(const Src& src, int32_t w, int32_t h, int32_t f, int32_t x, int32_t y, const float gp[8], const float B[4], const DenoiseSigma& sg,
                          float L[4], float out[4]) {
    int32_t x0, y0, rx, ry;
    upsample_split(x, f, x0, rx);
    upsample_split(y, f, y0, ry);
    float bx[4], by[4];
    upsample_spline((float)rx / (float)(2 * f), bx);
    upsample_spline((float)ry / (float)(2 * f), by);
    float Ne[3] = { 0.0f, 0.0f, 0.0f }, Ns[3] = { 0.0f, 0.0f, 0.0f }, De = 0.0f, Ds = 0.0f;
    for (int32_t j = 0; j < 4; ++j) {
        const int32_t ly = y0 - 1 + j;
        if (ly < 0 || ly >= h) continue;
        for (int32_t i = 0; i < 4; ++i) {
            const int32_t lx = x0 - 1 + i;
            if (lx < 0 || lx >= w) continue;
            float Lq[4], gq[8];
            src.tap(lx, ly, Lq, gq);
            const float s = bx[i] * by[j];
            const float se = s * upsample_edge(gp, gq, sg);
            for (int32_t c = 0; c < 3; ++c) {
                Ne[c] = Ne[c] + se * Lq[c];
                Ns[c] = Ns[c] + s * Lq[c];
            }
            De = De + se * Lq[3];
            Ds = Ds + s * Lq[3];
        }
    }
    const bool edge = De > kUpsampleMinWeight, spline = Ds > kUpsampleMinWeight;
    const float kappa = gp[3];
    float G[3];
    layers_background(B, kappa, G);
    for (int32_t c = 0; c < 3; ++c) {
        const float C = edge ? Ne[c] / De : (spline ? Ns[c] / Ds : 0.0f);
        L[c] = kappa * C;
        out[c] = max_(G[c] + L[c], 0.0f);
    }
    L[3] = kappa;
    out[3] = kappa;
}

}  // namespace vr
