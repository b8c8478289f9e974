// vr_layers.h -- the denoiser on the scattered layer alone, normalised by the expected coverage (host + device lane code).
//
// A partially covered pixel shows (1 - kappa) B + kappa C: the environment behind the volume and the scattered light.  kappa comes without noise from the
// expected-value feature pass (vr_expected.h), B analytically from vr_resolve.h's prepare; only C is noisy.  The a-trous filter on the composite blurs the
// sky's texture seen through thin smoke, and its coverage weight lets it mix pixels of different kappa, which smears the silhouette ramp that kappa already
// describes exactly.  With "denoise_layers" = 1 the filter runs on the scattered layer instead, and the analytic background goes back afterwards.
// Per-pixel functions only: the HIP kernels (vr_filters.hip layers_split_kernel, layers_merge_kernel) and the host build of the tests
// (tests/hostkernel/layers_host.cpp) run the same code, so the two agree bit for bit.  The arithmetic is fixed operation by operation (vr_math.h:
// -ffp-contract=off, IEEE division, max_); a * b + c below is two roundings.  All frames are W x H texels, row 0 at the bottom.
//
// Pixel p, with y_p the resolved frame (vr_resolve.h: alpha = kappa_p), B_p vr_resolve.h's background (0 with the environment hidden) and kappa_p the coverage
// channel of the feature buffer:
//   G_p     = (1 - kappa_p) * B_p, per channel: the background's share of the pixel.  Never stored: split and merge form it by this one expression.
// Split:
//   S_p.rgb = y_p.rgb - G_p   (signed, not clamped);   S_p.a = kappa_p
// Filter: vr_denoise.h's prepare, vr_temporal.h / vr_moments.h and the a-trous iterations, unchanged, on S in place of the frame, with the frame's own variance.
//   They filter channel 3 with the colour's weights, so F_p.a is kappa filtered by exactly the weights that filtered F_p.rgb.
// Merge, F the filter's output:
//   L_p.rgb = F_p.a > 2^-20 ? F_p.rgb * (kappa_p / F_p.a) : F_p.rgb;   L_p.a = kappa_p         the layer: scattered light premultiplied by the exact coverage
//   out.rgb = max_(G_p + L_p.rgb, 0);   out.a = kappa_p
// The normalisation matters: the premultiplied layer kappa C has a ramp across a silhouette that the composite hides when B ~ C; F.rgb / F.a is the filtered
// conditional mean C, and kappa_p puts the exact ramp back.  Zero iterations: F = S, the ratio is 1 (or not taken) and out = max_(G + (y - G), 0), y to two
// roundings.  A pixel with kappa = 0 whose filtered coverage exceeds 2^-20 -- the filter's footprint reached the volume -- has L.rgb = F.rgb * 0 = +-0 and
// G = 1 * B: it comes out as B bit for bit (B >= 0, finite F), the light the filter smeared onto it dropped.  Where the footprint met no coverage at all, F.a = 0
// and the pixel is B + the filtered (y - B): the filtered frame, as without the setting.  A caller composites L over any background B' as (1 - L.a) B' + L.rgb.
// Nothing is sanitised: a NaN in F makes the pixel NaN (max_(NaN, 0) is NaN).
//
// What it inherits.  kappa is the march's coverage: without a transfer function the tracker's lies about 0.0004 above it (vr_resolve.h), and that bias stays unless the pass marched the tracker's own field ("expected_field" 1).
// It needs what resolve() needs: an expected-value pass of rays >= 2, the whole frame, integrator != 2.
#pragma once

#include "vr_math.h"

namespace vr {

constexpr float kLayersMinWeight = 0x1p-20f;          // the smallest filtered coverage the merge divides by

// G: the background's share of the pixel
VR_HD void layers_background(const float B[4], float kappa, float G[3]) {
    const float omk = 1.0f - kappa;
    G[0] = omk * B[0];
    G[1] = omk * B[1];
    G[2] = omk * B[2];
}

// Split at a pixel: y its resolved texel, B its background texel, kappa its expected coverage -> S, what the filter reads in the frame's place
VR_HD void layers_split_pixel(const float y[4], const float B[4], float kappa, float S[4]) {
    float G[3];
    layers_background(B, kappa, G);
    S[0] = y[0] - G[0];
    S[1] = y[1] - G[1];
    S[2] = y[2] - G[2];
    S[3] = kappa;
}

// Merge at a pixel: F the filter's output there -> L the layer, out the frame with the background back
VR_HD void layers_merge_pixel(const float F[4], const float B[4], float kappa, float L[4], float out[4]) {
    float G[3];
    layers_background(B, kappa, G);
    const bool weighed = F[3] > kLayersMinWeight;
    const float r = weighed ? kappa / F[3] : 1.0f;
    for (int32_t c = 0; c < 3; ++c) {
        L[c] = weighed ? F[c] * r : F[c];
        out[c] = max_(G[c] + L[c], 0.0f);
    }
    L[3] = kappa;
    out[3] = kappa;
}

}  // namespace vr
