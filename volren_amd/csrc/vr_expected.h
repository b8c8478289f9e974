// vr_expected.h -- the denoiser's features as expected values: one deterministic ray march per pixel instead of a Monte-Carlo estimate.
//
// vr_trace.h feature_pixel averages first-scatter events, so its output is as noisy as the frame it guides.  None of its four quantities needs
// sampling: along a camera ray the first real collision has density p(t) = sigma(t) T(t), T the transmittance, and coverage, mean depth, mean albedo
// and mean normal are one-dimensional integrals of known functions.  expected_pixel marches the ray once and returns the limit of feature_pixel for
// spp -> infinity, in the same 8 floats (albedo.rgb, coverage, normal.xyz, depth), at a cost that does not depend on spp and without a random number:
// under a fixed camera and an unchanged scene the guide is bit-identical from frame to frame.
//
// The pass, operation by operation in float32 (this text is the specification; tests/hk_expected.py restates it in float64):
//   expected_pixel<TF>(P, px, py, n, out), n in 1..4: n x n sub-rays, j outer, i inner.
//   Sub-ray   feature_sample's camera expression with the jitters jx = ((float)i + 0.5f) / (float)n, jy = ((float)j + 0.5f) / (float)n.
//             intersect_box against vol_bb_min/max (the clip planes act through it, as in dvr_sample); ipos, idir through vol_density_inv_transform
//             as dvr_sample forms them.  A sub-ray contributes nothing when it misses the box, when !(tfar > tnear), or when L = length(idir) =
//             sqrt_(dot(idir, idir)), tnear or tfar is not finite.
//   Steps     m = clamp((int)ceil_((tfar - tnear) * L), 1, kExpectedMaxSteps), h = (tfar - tnear) / (float)m: at most one voxel per step, at most
//             4096 steps per sub-ray.  (The product is compared as a float before it is converted: a product beyond the int range, or one that
//             overflowed, gives kExpectedMaxSteps; one that is not above 1, 1.)  Step k samples the midpoint t = tnear + ((float)k + 0.5f) * h at
//             ip = axpy(ipos, t, idir).
//   Density   raw = the trilinear lookup (trilinear_prep / trilinear_load / trilinear_value) of P.density at ip.  Without a LUT sigma =
//             vol_density_scale * raw and a = vol_albedo; with one, tf_lookup(P, (vol_density_scale * raw) * vol_inv_majorant, rgba), sigma = rgba[3] *
//             vol_majorant, a = vol_albedo * rgba.rgb.  A step with !(sigma > 0) -- NaN included -- contributes nothing and leaves T as it is.
//             Without a LUT the tracker of feature_sample decides its collisions on the stochastic-tricubic (B-spline) field, about a voxel smoother
//             than the trilinear one marched here: the two passes agree up to that difference.
//   Weights   e = exp_(-(sigma * h)), w = T * (1 - e), then T = T * e.  The sub-ray ends when T <= 2^-10 (kExpectedMinT): what is left of it is
//             below the precision the filter's edge weights resolve.
//   Normal    g = trilinear_gradient of the same eight corners (vr_trace.h; no further loads), n^ = -normalize(transpose(Minv3) g) in
//             feature_sample's expression, 0 where it vanishes.  (feature_sample takes a central difference one voxel each way.)
//   Sums      float32, in step order, then sub-ray order: K += w, D += w * t, A += w * a, N += w * n^ (each product rounded, then the sum).
//   Output    albedo = A / K, coverage = K / (float)(n * n), normal = N / K (not renormalised, as in feature_pixel), depth = D / K; all eight
//             zero when !(K > 0).  t is the distance along the unit camera ray, as in feature_sample.
// The emission grid, the integrator setting and the majorant table play no part; nothing is skipped: a step in empty space loads its eight corners and
// adds nothing.
#pragma once

#include "vr_trace.h"

namespace vr {

constexpr int32_t kExpectedMaxSteps = 4096;          // per sub-ray
constexpr float kExpectedMinT = 1.0f / 1024.0f;

struct ExpectedSums { float K, D; v3 A, N; };
// what a test harness may want to know of one sub-ray: its step count (0: it contributed nothing), the steps it ran, and the transmittance it ended with
struct ExpectedRayInfo { int32_t m, steps; float T; };

VR_HD bool expected_finite(float x) { return abs_(x) < inf_(); }

template <bool TF, bool INFO = false>
VR_HD void expected_subray(const SceneParams& P, int32_t px, int32_t py, int32_t i, int32_t j, int32_t n, ExpectedSums& S, ExpectedRayInfo* info = nullptr) {
    const Uniforms& u = P.u;
    const int32_t W = u.resolution[0], H = u.resolution[1];
    if (INFO) { info->m = 0; info->steps = 0; info->T = 1.0f; }
    const float jx = ((float)i + 0.5f) / (float)n, jy = ((float)j + 0.5f) / (float)n;
    const float fx = (((float)px + jx) - (float)W * 0.5f) / (float)H;
    const float fy = (((float)py + jy) - (float)H * 0.5f) / (float)H;
    const v3 dir = normalize(mat3_mul(u.cam_transform, normalize(v3{ fx, fy, P.cam_z })));
    const v3 pos = v3{ u.cam_pos[0], u.cam_pos[1], u.cam_pos[2] };
    float tnear, tfar;
    if (!intersect_box(pos, dir, u.vol_bb_min, u.vol_bb_max, tnear, tfar)) return;
    const v3 ipos = mat4_point(u.vol_density_inv_transform, pos);
    const v3 idir = mat4_dir(u.vol_density_inv_transform, dir);
    const float L = sqrt_(dot(idir, idir));
    if (!(tfar > tnear) || !expected_finite(L) || !expected_finite(tnear) || !expected_finite(tfar)) return;
    const float len = tfar - tnear, mf = ceil_(len * L);
    const int32_t m = mf >= (float)kExpectedMaxSteps ? kExpectedMaxSteps : (mf >= 1.0f ? (int32_t)mf : 1);
    const float h = len / (float)m;
    const v3 alb = v3{ u.vol_albedo[0], u.vol_albedo[1], u.vol_albedo[2] };
    const float* mi = u.vol_density_inv_transform;         // column-major: row i of transpose(Minv3) = column i of Minv3
    float T = 1.0f;
    int32_t k = 0;
    for (; k < m; ++k) {
        const float t = tnear + ((float)k + 0.5f) * h;
        TriIO io;
        trilinear_prep(P.density, axpy(ipos, t, idir), io);
        trilinear_load(P.density, io);
        const float raw = trilinear_value(P.density, io);
        float sigma = u.vol_density_scale * raw;
        v3 a = alb;
        if (TF) {
            float rgba[4];
            tf_lookup(P, sigma * u.vol_inv_majorant, rgba);
            sigma = rgba[3] * u.vol_majorant;
            a = alb * v3{ rgba[0], rgba[1], rgba[2] };
        }
        if (!(sigma > 0.0f)) continue;
        const float e = exp_(-(sigma * h));
        const float w = T * (1.0f - e);
        T = T * e;
        const v3 g = trilinear_gradient(P.density, io);
        const v3 nn = v3{ (mi[0] * g.x + mi[1] * g.y) + mi[2] * g.z, (mi[4] * g.x + mi[5] * g.y) + mi[6] * g.z, (mi[8] * g.x + mi[9] * g.y) + mi[10] * g.z };
        const v3 nh = (nn.x == 0.0f && nn.y == 0.0f && nn.z == 0.0f) ? v3{ 0, 0, 0 } : -normalize(nn);
        S.K += w;
        S.D += w * t;
        S.A = S.A + a * w;
        S.N = S.N + nh * w;
        if (T <= kExpectedMinT) { ++k; break; }
    }
    if (INFO) { info->m = m; info->steps = k; info->T = T; }
}

// info (INFO only): n * n entries, sub-ray j * n + i
template <bool TF, bool INFO = false>
VR_HD void expected_pixel(const SceneParams& P, int32_t px, int32_t py, int32_t n, float out[8], ExpectedRayInfo* info = nullptr) {
    ExpectedSums S;
    S.K = 0.0f; S.D = 0.0f; S.A = v3{ 0, 0, 0 }; S.N = v3{ 0, 0, 0 };
    for (int32_t j = 0; j < n; ++j)
        for (int32_t i = 0; i < n; ++i) expected_subray<TF, INFO>(P, px, py, i, j, n, S, INFO ? info + (j * n + i) : nullptr);
    for (int32_t c = 0; c < 8; ++c) out[c] = 0.0f;
    if (!(S.K > 0.0f)) return;
    out[0] = S.A.x / S.K; out[1] = S.A.y / S.K; out[2] = S.A.z / S.K; out[3] = S.K / (float)(n * n);
    out[4] = S.N.x / S.K; out[5] = S.N.y / S.K; out[6] = S.N.z / S.K; out[7] = S.D / S.K;
}

}  // namespace vr
