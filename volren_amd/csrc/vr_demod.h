// vr_demod.h -- the scattered layer demodulated by the guide's exact albedo around the filter (host + device lane code).
//
// Every scattered sample is a_1 * R: a_1 the albedo of the path's first collision (vol_albedo times the transfer function's colour there), R everything after it.
// Under a transfer function a_1 carries the sharp colour texture and R is smooth, but vr_layers.h's S = kappa C is their product, and the filter's albedo weight
// w_a has to stop at every colour edge of the LUT.  The expected-value pass (vr_expected.h) gives the pixel's mean first-scatter albedo A / K without noise: words
// 0..2 of the feature buffer.  With "denoise_demodulate" = 1 (needs "denoise_layers" = 1) the split divides S by it, the filter runs on the quotient, and the merge
// multiplies it back: the standard demodulation of SVGF (Schied et al. 2017), with the albedo of a volume's first scatter in the surface albedo's place.
// Per-pixel functions only: the HIP kernels (vr_filters.hip, the DEMOD instances of layers_split_kernel, layers_merge_kernel, denoise_prepare_kernel and
// upsample_kernel) and the host build of the tests (tests/hostkernel/demod_host.cpp) run the same code, so the two agree bit for bit.  The arithmetic is fixed
// operation by operation (vr_math.h: -ffp-contract=off, IEEE division, sqrt_, max_, luma); a * b + c below is two roundings.
//
// Pixel p, (a_p, kappa_p) words 0..2 and 3 of its features (of its guide: vr_denoise.h's guide copies them), y, B, G as in vr_layers.h:
// Divisor, per channel c:
//   d_c = kappa_p > 0 ? max_(a_c, kDemodFloor) : 1;   kDemodFloor = 2^-6
//   Nothing is sanitised: a NaN albedo gives a NaN divisor (vr_math.h max_(x, y) is x < y ? y : x, and NaN < floor is false) and with it a NaN pixel; an
//   infinite albedo divides to 0.
// Split:
//   S_p.rgb = (y_p.rgb - G_p) / d        layers_split_pixel, then one IEEE division per channel;   S_p.a = kappa_p
// Variance (prepare), var the unbiased per-channel variance, w luma's weights, n the samples:
//   t_c = sqrt_(max_(var_c, 0)) / d_c;   s = luma(t);   v_p = (s * s) / float(n)
//   denoise_mean_variance with every channel's standard deviation divided by d_c: the variance of the demodulated mean's luminance under that function's
//   assumption (perfectly correlated channels).  With d = 1 it is that function bit for bit (x / 1 = x).
// Filter: vr_denoise.h's iterations or vr_regress.h's pass, vr_temporal.h's blend and rejection and vr_moments.h read the demodulated S and v unchanged; the
//   history holds the demodulated layer.
// Merge, F the filter's output:
//   L = layers_merge_pixel's L of F (the normalisation by kappa_p / F.a);   L.rgb = L.rgb * d;   out.rgb = max_(G_p + L.rgb, 0);   L.a = out.a = kappa_p
//   The layer keeps its meaning: scattered light premultiplied by the exact coverage, remodulated.  Zero iterations: F = S and out = max_(G + ((y - G) / d) * d, 0).
//   kappa_p = 0: d = 1, so S, v and the merge are vr_layers.h's own, operation by operation and bit for bit (x / 1 = x, x * 1 = x, signed zeros included): the
//   pixel comes out as B where it does there (F.a > 2^-20: L.rgb = F.rgb * 0 = +-0, +-0 * 1 = +-0, G = 1 * B, max_(B + +-0, 0) = B for B >= 0), and as the
//   filtered frame where the footprint met no coverage.
// Upsample (vr_upsample.h): the taps hand out L_q.rgb / d_q, d_q from the lo guide (DemodTaps below; the kernel divides once when it stages a lo record, the
//   same values), upsample_pixel runs unchanged on them, and its hi layer kappa_p * C is remodulated: L_p.rgb = (kappa_p * C) * d_p, d_p from the hi guide,
//   out.rgb = max_(G_p + L_p.rgb, 0).  The lo layer is re-demodulated inside the call, so the call demodulates exactly when the setting is 1 at the call,
//   whatever produced the layer.
//
// What the floor costs.  A channel with a_c < floor is divided by the floor, not by a_c: its quotient is (a_c / floor) R, not R, and after the filter mixed it with
// its neighbours' R' and the merge multiplied by the floor again, the pixel keeps at most floor * R' of the neighbours' irradiance where a_c * R' would be right --
// a bias of at most floor * (the neighbours' irradiance) per channel, 1.6 % of it.  Light that carries no a_1 -- an emission grid's, added along the path -- is
// divided all the same: where the albedo is small it is amplified by at most 1 / floor = 64 before the filter, and its noise with it.  The result stays valid
// (the merge multiplies back), but such a pixel dominates its neighbours' colour weight.  Emission-aware demodulation is not built.
#pragma once

#include "vr_denoise.h"
#include "vr_layers.h"
#include "vr_math.h"
#include "vr_upsample.h"

namespace vr {

constexpr float kDemodFloor = 0x1p-6f;                // the smallest albedo the layer is divided by

// d of a pixel from words 0..3 of its features (or of its guide): albedo.rgb, coverage
VR_HD void demod_divisor(const float ak[4], float d[3]) {
    const bool covered = ak[3] > 0.0f;
    d[0] = covered ? max_(ak[0], kDemodFloor) : 1.0f;
    d[1] = covered ? max_(ak[1], kDemodFloor) : 1.0f;
    d[2] = covered ? max_(ak[2], kDemodFloor) : 1.0f;
}

// Split at a pixel: layers_split_pixel, then the division.  ak = words 0..3 of the pixel's features
VR_HD void demod_split_pixel(const float y[4], const float B[4], const float ak[4], float S[4]) {
    float d[3];
    demod_divisor(ak, d);
    layers_split_pixel(y, B, ak[3], S);
    S[0] = S[0] / d[0];
    S[1] = S[1] / d[1];
    S[2] = S[2] / d[2];
}

// prepare's v of the demodulated layer: var the unbiased per-channel variance of n >= 1 samples
VR_HD float demod_mean_variance(const float var[4], const float ak[4], int32_t n) {
    float d[3];
    demod_divisor(ak, d);
    const float s = luma(v3{ sqrt_(max_(var[0], 0.0f)) / d[0], sqrt_(max_(var[1], 0.0f)) / d[1], sqrt_(max_(var[2], 0.0f)) / d[2] });
    return (s * s) / (float)n;
}

// Merge at a pixel: layers_merge_pixel's L of F, remodulated; out with the background back
VR_HD void demod_merge_pixel(const float F[4], const float B[4], const float ak[4], float L[4], float out[4]) {
    float d[3], G[3], plain[4];
    demod_divisor(ak, d);
    layers_merge_pixel(F, B, ak[3], L, plain);
    layers_background(B, ak[3], G);
    for (int32_t c = 0; c < 3; ++c) {
        L[c] = L[c] * d[c];
        out[c] = max_(G[c] + L[c], 0.0f);
    }
    out[3] = ak[3];
}

// a lo tap's layer texel demodulated by the tap's own guide: what the taps of the upsampling hand out
VR_HD void demod_tap(float L[4], const float g[8]) {
    float d[3];
    demod_divisor(g, d);
    L[0] = L[0] / d[0];
    L[1] = L[1] / d[1];
    L[2] = L[2] / d[2];
}
// the Src of upsample_pixel over another Src: every tap demodulated as it is read
template <class Src>
struct DemodTaps {
    Src src;
    VR_HD void tap(int32_t lx, int32_t ly, float L[4], float g[8]) const {
        src.tap(lx, ly, L, g);
        demod_tap(L, g);
    }
};

// Hi pixel of the upsampling: src hands out DEMODULATED lo texels (DemodTaps, or a window staged through demod_tap); gp the pixel's hi guide
template <class Src>
VR_HD void demod_upsample_pixel(const Src& src, int32_t w, int32_t h, int32_t f, int32_t x, int32_t y, const float gp[8], const float B[4], const DenoiseSigma& sg,
                                float L[4], float out[4]) {
    float d[3], G[3], plain[4];
    demod_divisor(gp, d);
    upsample_pixel(src, w, h, f, x, y, gp, B, sg, L, plain);
    layers_background(B, gp[3], G);
    for (int32_t c = 0; c < 3; ++c) {
        L[c] = L[c] * d[c];
        out[c] = max_(G[c] + L[c], 0.0f);
    }
    out[3] = gp[3];
}

}  // namespace vr
