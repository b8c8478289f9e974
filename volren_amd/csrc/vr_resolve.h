// vr_resolve.h -- the frame's hit/miss noise replaced by the expected coverage: a control variate in image space (host + device lane code).
//
// trace_path returns alpha = 1 for a sample that scattered at least once and 0 for one that flew through, so the framebuffer's alpha is kappa^, the
// share of the pixel's n samples that hit.  The expected-value feature pass (vr_expected.h) gives the same number without noise: kappa, the exact
// probability that a camera sample collides.  In a partially covered pixel a sample is either the environment behind the volume (radiance B) or
// scattered light (conditional mean C), and which of the two is a coin toss of variance kappa (1 - kappa) (B - C)^2 per sample.  The toss's expectation
// is known, so it serves as a control variate:
//     y = x + beta (kappa^ - kappa),   beta = B - C~
// x the frame's mean, C~ an estimate of C pooled over the pixel's neighbourhood.  Per-pixel functions only: the HIP kernels (vr_filters.hip
// resolve_prepare_kernel, resolve_kernel) and the host build of the tests (tests/hostkernel/resolve_host.cpp) run the same code, so the two agree bit
// for bit.  The arithmetic is fixed operation by operation (vr_math.h: -ffp-contract=off, IEEE division, max_); a * b + c below is two roundings.
// All frames are W x H texels, row 0 at the bottom.
//
// Prepare, pixel p, with n = the rays of the expected pass that filled the feature buffer:
//   B_p   = (sum over the n x n sub-rays, j outer, i inner, from 0, of lookup_environment(dir_ij)) / (float)(n * n), per channel; dir_ij the sub-ray's
//           direction: feature_sample's camera expression with the jitters jx = ((float)i + 0.5f) / (float)n, jy = ((float)j + 0.5f) / (float)n --
//           vr_expected.h's sub-rays, every one of them, whether it meets the volume's box or not.  lookup_environment (vr_trace.h) is what the path
//           tracer adds for a camera ray that escapes: strength and transform included.  B_p = 0 when show_environment is 0 (nothing is looked up).
//   kappa^_p = x_p.a;   P_p = (x_p.rgb - (1 - kappa^_p) * B_p, kappa^_p): the frame's scattered part and its weight.
//   Stored: B (W*H*4, .a = 0) and P (W*H*4).
// Resolve, pixel p, kappa_p the coverage channel of the feature buffer:
//   (N.rgb, D) = sum of P_q over q = p + (dx, dy), dx, dy in -3 .. 3, dy outer, dx inner, each sum from 0, taps outside the frame skipped
//   C~ = D > 0 ? N / D : 0   (per channel; a NaN D gives 0);   beta = B_p - C~
//   y.rgb = max_(x_p.rgb + beta * (kappa^_p - kappa_p), 0);   y.a = kappa_p
// A pixel with kappa^_p = kappa_p keeps its rgb bit for bit (beta finite: beta * 0 = +-0, x + +-0 = x, and max_(x, 0) = x for x >= 0); a window without
// any hit has D = 0 and beta = B_p.  Nothing is sanitised: a NaN in the frame makes the pixels whose window holds it NaN (max_(NaN, 0) is NaN, vr_math.h:
// x < y ? y : x).
//
// What the estimator assumes.  E[y] = E[x] + beta (E[kappa^] - kappa) for a fixed beta: y is unbiased wherever the path tracer's tracker collides with
// the probability the march integrates.  Under a transfer function it does: the tracker decides its collisions on the very field -- trilinear density
// through the LUT -- that expected_pixel marches.  Without one the tracker uses the stochastic-tricubic (B-spline) field, about a voxel smoother; the two
// coverages differ by about 0.002 on average, and y carries beta times that difference as bias -- unless the pass marched that field itself
// ("expected_field" 1: vr_expected.h CUBIC), where the coverages agree to within sampling noise.  beta itself is estimated from the frame (C~), which
// couples it to kappa^: a second-order bias that shrinks with the 49 pixels pooled and with the sample count.  With an emission grid the estimator stays
// valid -- emission before the first collision is part of x and of B's complement alike -- but beta is no longer the optimal coefficient.  The direct
// volume rendering integrator (2) writes an opacity into alpha, not a hit indicator: the renderer refuses it.  kappa from one ray per pixel is the
// coverage of the pixel's centre, not of its area: the renderer refuses rays < 2.
#pragma once

#include "vr_trace.h"

namespace vr {

constexpr int32_t kResolveWindow = 3;                 // C~ pools a (2 * 3 + 1)^2 window

// B_p: the mean environment radiance behind the pixel, over vr_expected.h's n x n sub-rays
VR_HD v3 resolve_background(const SceneParams& P, int32_t px, int32_t py, int32_t n) {
    const Uniforms& u = P.u;
    v3 s = v3{ 0.0f, 0.0f, 0.0f };
    if (!(u.show_environment > 0)) return s;
    const int32_t W = u.resolution[0], H = u.resolution[1];
    for (int32_t j = 0; j < n; ++j)
        for (int32_t i = 0; i < n; ++i) {
            const float jx = ((float)i + 0.5f) / (float)n, jy = ((float)j + 0.5f) / (float)n;
            const float fx = (((float)px + jx) - (float)W * 0.5f) / (float)H;
            const float fy = (((float)py + jy) - (float)H * 0.5f) / (float)H;
            const v3 dir = normalize(mat3_mul(u.cam_transform, normalize(v3{ fx, fy, P.cam_z })));
            s = s + lookup_environment(P, dir);
        }
    const float nn = (float)(n * n);
    return v3{ s.x / nn, s.y / nn, s.z / nn };
}

// Prepare at a pixel: x its framebuffer texel, b its B_p.  Bout / Pout: the pixel's texels of the two stored frames
VR_HD void resolve_prepare_pixel(const float x[4], v3 b, float Bout[4], float Pout[4]) {
    const float kh = x[3], omk = 1.0f - kh;
    Bout[0] = b.x; Bout[1] = b.y; Bout[2] = b.z; Bout[3] = 0.0f;
    Pout[0] = x[0] - omk * b.x;
    Pout[1] = x[1] - omk * b.y;
    Pout[2] = x[2] - omk * b.z;
    Pout[3] = kh;
}

// Resolve at pixel (px, py): x its framebuffer texel, B its B_p, kappa its expected coverage.  Win answers  void tap(int32_t dx, int32_t dy, float p[4]) const:
// P of pixel p + (dx, dy), asked only for pixels inside the frame.
template <class Win>
VR_HD void resolve_pixel(const Win& win, int32_t W, int32_t H, int32_t px, int32_t py, const float x[4], const float B[4], float kappa, float y[4]) {
    float N[3] = { 0.0f, 0.0f, 0.0f }, D = 0.0f;
    for (int32_t dy = -kResolveWindow; dy <= kResolveWindow; ++dy)
        for (int32_t dx = -kResolveWindow; dx <= kResolveWindow; ++dx) {
            const int32_t qx = px + dx, qy = py + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            float p[4];
            win.tap(dx, dy, p);
            N[0] = N[0] + p[0];
            N[1] = N[1] + p[1];
            N[2] = N[2] + p[2];
            D = D + p[3];
        }
    const bool hit = D > 0.0f;
    const float dk = x[3] - kappa;
    for (int32_t c = 0; c < 3; ++c) {
        const float Ct = hit ? N[c] / D : 0.0f;
        const float beta = B[c] - Ct;
        y[c] = max_(x[c] + beta * dk, 0.0f);
    }
    y[3] = kappa;
}

}  // namespace vr
