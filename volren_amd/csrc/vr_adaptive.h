// vr_adaptive.h -- adaptive sampling per 16x16 tile: the error estimate (host + device lane code) and the schedule (host).
//
// The error kernel (vr_filters.hip adaptive_error_kernel) and the host build of the tests (tests/hostkernel/adaptive_host.cpp) run the same
// code, so the two agree bit for bit.  The arithmetic is fixed operation by operation (vr_math.h: -ffp-contract=off, IEEE division, sqrt_, luma).
// For a pixel with n samples, framebuffer mean mu (RGBA) and moments S (Welford's M2 / n, what the renderer's moments hold):
//   var_c = n >= 2 ? S_c * variance_scale(n) : 0                  vr_variance's and denoise_prepare_kernel's formation (vr_tiles.h)
//   e_p   = n < 2 ? +inf : sqrt_(denoise_mean_variance(var, n)) / (luma(mu.rgb) + kAdaptiveFloor)
//   e_t   = the max of e_p over the tile's pixels inside the frame; a NaN e_p makes e_t NaN
// e_t is the worst relative standard error of a pixel mean's luminance in the tile.  Tile t has converged iff e_t < threshold (strict:
// threshold 0 never converges, NaN never does).
//
// Schedule (RendererHIP::render_adaptive): the tiles of the tile set are first brought to min_spp; then, while some tile of the set has fewer
// than max_spp samples, one round evaluates e_t of those (one launch), retires the converged ones, and takes every other from n_t to
// adaptive_next_count(n_t) = min(2 n_t, max_spp) -- one path-tracing submit per group of equal n_t (adaptive_groups).
#pragma once

#include <map>
#include <vector>

#include "vr_denoise.h"
#include "vr_tiles.h"

namespace vr {

constexpr float kAdaptiveFloor = 0x1p-10f;       // keeps e_p finite on black pixels: their error is taken relative to 2^-10

// max that propagates NaN (as a canonical quiet NaN); identity -inf
VR_HD float adaptive_max(float a, float b) { return (a != a || b != b) ? nan_() : max_(a, b); }

// e_p of a pixel of n >= 2 samples from its unbiased variance var (what vr_variance returns)
VR_HD float adaptive_error_of_variance(const float mu[4], const float var[4], int32_t n) {
    return sqrt_(denoise_mean_variance(var, n)) / (luma(v3{ mu[0], mu[1], mu[2] }) + kAdaptiveFloor);
}

// e_p of one pixel: mu = the framebuffer texel, S = the moments texel, n = the samples behind both
VR_HD float adaptive_pixel_error(const float mu[4], const float S[4], int32_t n) {
    if (n < 2) return inf_();
    const float f = variance_scale(n);
    const float var[4] = { S[0] * f, S[1] * f, S[2] * f, S[3] * f };
    return adaptive_error_of_variance(mu, var, n);
}

VR_HD bool adaptive_converged(float e, float threshold) { return e < threshold; }

// the count an active tile of n samples goes to next: min(2 n, max_spp), without overflow
VR_HD int32_t adaptive_next_count(int32_t n, int32_t max_spp) { return n >= max_spp - n ? max_spp : 2 * n; }

// the tiles of `ids` grouped by their count (counts indexed by raster tile id): ascending counts, each group in the order of `ids`
inline std::map<int32_t, std::vector<int32_t>> adaptive_groups(const std::vector<int32_t>& ids, const std::vector<int32_t>& counts) {
    std::map<int32_t, std::vector<int32_t>> g;
    for (int32_t t : ids) g[counts[(size_t)t]].push_back(t);
    return g;
}

}  // namespace vr
