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
//             than the trilinear one marched here: the two passes agree up to that difference (coverage: 4e-4 on smoke.brick, 6e-3 on a dense 64^3
//             grid), which CUBIC removes.
//   CUBIC     (without a LUT; with one the tracker itself looks up the trilinear field, and CUBIC changes nothing.)  The Density line reads raw =
//             the cubic B-spline field of vr_cubic.h (cubic_lookup: 64 taps, fl - 1 .. fl + 2 per axis, fl = floor(ip - 0.5)) instead, the mean of
//             the tracker's stochastic tap, and the Normal line takes g from the same lookup -- the same 64 values, no further loads -- through the
//             same transpose(Minv3), normalise and negate.  Everything else is the text as it stands.
//   Weights   e = exp_(-(sigma * h)), w = T * (1 - e), then T = T * e.  The sub-ray ends when T <= 2^-10 (kExpectedMinT): what is left of it is
//             below the precision the filter's edge weights resolve.
//   Normal    g = trilinear_gradient of the same eight corners (vr_trace.h; no further loads), n^ = -normalize(transpose(Minv3) g) in
//             feature_sample's expression, 0 where it vanishes.  (feature_sample takes a central difference one voxel each way.)
//   Sums      float32, in step order, then sub-ray order: K += w, D += w * t, A += w * a, N += w * n^ (each product rounded, then the sum).
//   Output    albedo = A / K, coverage = K / (float)(n * n), normal = N / K (not renormalised, as in feature_pixel), depth = D / K; all eight
//             zero when !(K > 0).  t is the distance along the unit camera ray, as in feature_sample.
// The emission grid, the integrator setting and the majorant table play no part.
//
// Empty space (SKIP, with the clear-distance table of vr_clear.h; without one the march is the text above, step by step).  A step whose eight corners
// are all +0 (CUBIC: whose 64 taps are all +0) has raw = +0 whatever its weights, so its sigma is the value s0 of the Density line at raw = +0.0f; when !(s0 > 0) -- always without a LUT:
// vol_density_scale * (+0) is +-0 or NaN; with one unless the LUT's alpha at density 0 is positive -- such a step contributes nothing and may be
// dropped with its loads.  s0 is evaluated once per pixel; when it is > 0 the pixel marches every step.  Otherwise step k, before it loads anything,
// reads the byte d of the cell that holds its midpoint ip, cell floor(ip / 8) per axis:
//   ip outside the table (NaN included) or d == 0: the step runs as above.
//   d >= 1: the cell is clear, the corners -- floor(ip - 0.5) and one more per axis -- lie in its grown box: the step is dropped.  And it leaps: the
//           midpoints of a sub-ray whose m is not capped move h |idir_i| <= h L <= 1 voxel per step and axis, so the next 7 (d - 1) of them lie
//           less than 8 (d - 1) voxels from this one, within d - 1 cells of its cell, which are all clear (or outside the grid): k += 1 + 7 (d - 1),
//           and the table is read again where that lands.  The eighth of a cell per cell is the margin against rounding, which is why a sub-ray
//           leaps only while max |ipos_i| + tfar max |idir_i| < 2^16 (kExpectedLeapBound): there a midpoint is computed to within 0.02 voxels.
//           Every other sub-ray -- m capped at kExpectedMaxSteps, or coordinates beyond that bound -- drops one step at a time.
// CUBIC marches with the table of reach 2 (vr_clear.h): ip in [8 c, 8 c + 8) gives fl in [8 c - 1, 8 c + 7], taps in [8 c - 2, 8 c + 9], the cell's box grown by
// two voxels.  A clear cell gives 64 taps of +0, a sum of products with +0 -- raw = +0, or NaN under weights that are not finite --, hence !(sigma > 0); the leap
// argument holds unchanged.
// The frame is the same bits with and without the table.  ExpectedRayInfo::steps stays the step index the sub-ray reached, dropped steps included
// (a leap past the last step ends at m).
#pragma once

#include "vr_clear.h"
#include "vr_cubic.h"
#include "vr_trace.h"

namespace vr {

constexpr int32_t kExpectedMaxSteps = 4096;          // per sub-ray
constexpr float kExpectedMinT = 1.0f / 1024.0f;

struct ExpectedSums { float K, D; v3 A, N; };
// what a test harness may want to know of one sub-ray: its step count (0: it contributed nothing), the steps it ran, and the transmittance it ended with
struct ExpectedRayInfo { int32_t m, steps; float T; };

// what an instrumented pass counts, summed over the sub-rays it is handed to: sub-rays marched (m > 0), the step indices they reached
// (ExpectedRayInfo::steps), the steps that fetched their corners, the reads of the clear-distance table; audit (host harness only): dropped steps
// that, evaluated in full, have sigma > 0 -- none, if the table is what vr_clear.h says
struct ExpectedWork { uint32_t rays, steps, fetched, reads, audit; };
constexpr float kExpectedLeapBound = 65536.0f;

VR_HD bool expected_finite(float x) { return abs_(x) < inf_(); }

// the Density line: sigma and albedo of the step at ip, its corners left in io for the normal
template <bool TF>
VR_HD float expected_sigma(const SceneParams& P, v3 ip, v3 alb, TriIO& io, v3& a) {
    const Uniforms& u = P.u;
    trilinear_prep(P.density, ip, io);
    trilinear_load(P.density, io);
    const float raw = trilinear_value(P.density, io);
    float sigma = u.vol_density_scale * raw;
    a = alb;
    if (TF) {
        float rgba[4];
        tf_lookup(P, sigma * u.vol_inv_majorant, rgba);
        sigma = rgba[3] * u.vol_majorant;
        a = alb * v3{ rgba[0], rgba[1], rgba[2] };
    }
    return sigma;
}
// CUBIC's Density line (no LUT): sigma of the step at ip, the gradient of the same 64 taps in g
VR_HD float expected_sigma_cubic(const SceneParams& P, v3 ip, v3& g) {
    float raw;
    cubic_lookup(P.density, ip, raw, g);
    return P.u.vol_density_scale * raw;
}
// the same line at raw = +0.0f: the sigma of every step whose eight corners are +0
template <bool TF>
VR_HD float expected_sigma_of_zero(const SceneParams& P) {
    const Uniforms& u = P.u;
    float sigma = u.vol_density_scale * 0.0f;
    if (TF) {
        float rgba[4];
        tf_lookup(P, sigma * u.vol_inv_majorant, rgba);
        sigma = rgba[3] * u.vol_majorant;
    }
    return sigma;
}

// SKIP: with clear (its table not null) and skip (the pixel's !(expected_sigma_of_zero > 0)) steps in clear cells are dropped; WORK: work counts;
// AUDIT (host only, with WORK): every dropped step is evaluated all the same and counted in work->audit when its sigma > 0; CUBIC: the cubic B-spline
// field (without a LUT; clear must then be the table of reach 2)
template <bool TF, bool INFO = false, bool SKIP = false, bool WORK = false, bool AUDIT = false, bool CUBIC = false>
VR_HD void expected_subray(const SceneParams& P, int32_t px, int32_t py, int32_t i, int32_t j, int32_t n, ExpectedSums& S, ExpectedRayInfo* info = nullptr,
                           const ClearTable* clear = nullptr, bool skip = false, ExpectedWork* work = nullptr) {
    constexpr bool CB = CUBIC && !TF;
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
    bool leap = false;
    float lim[3] = { 0.0f, 0.0f, 0.0f };
    if (SKIP && skip) {
        const float reach = max_(max_(abs_(ipos.x), abs_(ipos.y)), abs_(ipos.z)) + tfar * max_(max_(abs_(idir.x), abs_(idir.y)), abs_(idir.z));
        leap = m < kExpectedMaxSteps && reach < kExpectedLeapBound;
        for (int c = 0; c < 3; ++c) lim[c] = (float)(clear->n[c] << 3);
    }
    float T = 1.0f;
    int32_t k = 0;
    for (; k < m; ++k) {
        const float t = tnear + ((float)k + 0.5f) * h;
        const v3 ip = axpy(ipos, t, idir);
        TriIO io;
        v3 a = alb, g;
        if (SKIP && skip) {
            // (One loop over fetched and dropped steps alike: neighbouring rays cross the same cells nearly in lockstep, so a wavefront mostly drops or fetches as
            // one.  A loop of its own that runs each lane ahead to its next fetching step measured slower: profiles/r12_expected_skip.txt.)
            // inside the table on the floats (NaN fails), after which truncation is floor
            if ((ip.x >= 0.0f) & (ip.x < lim[0]) & (ip.y >= 0.0f) & (ip.y < lim[1]) & (ip.z >= 0.0f) & (ip.z < lim[2])) {
                const uint32_t cx = (uint32_t)(int32_t)ip.x >> 3, cy = (uint32_t)(int32_t)ip.y >> 3, cz = (uint32_t)(int32_t)ip.z >> 3;
                const uint32_t d = clear->d[(cz * (uint32_t)clear->n[1] + cy) * (uint32_t)clear->n[0] + cx];
                if (WORK) ++work->reads;
                if (d != 0u) {
                    const int32_t more = leap ? 7 * ((int32_t)d - 1) : 0;
                    if (AUDIT)
                        for (int32_t kk = k; kk <= k + more && kk < m; ++kk)
                            if ((CB ? expected_sigma_cubic(P, axpy(ipos, tnear + ((float)kk + 0.5f) * h, idir), g)
                                    : expected_sigma<TF>(P, axpy(ipos, tnear + ((float)kk + 0.5f) * h, idir), alb, io, a)) > 0.0f) ++work->audit;
                    k += more;
                    continue;
                }
            }
        }
        if (WORK) ++work->fetched;
        const float sigma = CB ? expected_sigma_cubic(P, ip, g) : expected_sigma<TF>(P, ip, alb, io, a);
        if (!(sigma > 0.0f)) continue;
        const float e = exp_(-(sigma * h));
        const float w = T * (1.0f - e);
        T = T * e;
        if (!CB) g = trilinear_gradient(P.density, io);
        const v3 nn = v3{ (mi[0] * g.x + mi[1] * g.y) + mi[2] * g.z, (mi[4] * g.x + mi[5] * g.y) + mi[6] * g.z, (mi[8] * g.x + mi[9] * g.y) + mi[10] * g.z };
        const v3 nh = (nn.x == 0.0f && nn.y == 0.0f && nn.z == 0.0f) ? v3{ 0, 0, 0 } : -normalize(nn);
        S.K += w;
        S.D += w * t;
        S.A = S.A + a * w;
        S.N = S.N + nh * w;
        if (T <= kExpectedMinT) { ++k; break; }
    }
    if (SKIP && k > m) k = m;                              // a leap past the last step
    if (INFO) { info->m = m; info->steps = k; info->T = T; }
    if (WORK) { ++work->rays; work->steps += (uint32_t)k; }
}

// info (INFO only): n * n entries, sub-ray j * n + i
template <bool TF, bool INFO = false, bool SKIP = false, bool WORK = false, bool AUDIT = false, bool CUBIC = false>
VR_HD void expected_pixel(const SceneParams& P, int32_t px, int32_t py, int32_t n, float out[8], ExpectedRayInfo* info = nullptr,
                          const ClearTable* clear = nullptr, ExpectedWork* work = nullptr) {
    ExpectedSums S;
    S.K = 0.0f; S.D = 0.0f; S.A = v3{ 0, 0, 0 }; S.N = v3{ 0, 0, 0 };
    const bool skip = SKIP && clear && clear->d && !(expected_sigma_of_zero<TF>(P) > 0.0f);
    for (int32_t j = 0; j < n; ++j)
        for (int32_t i = 0; i < n; ++i) expected_subray<TF, INFO, SKIP, WORK, AUDIT, CUBIC>(P, px, py, i, j, n, S, INFO ? info + (j * n + i) : nullptr, clear, skip, work);
    for (int32_t c = 0; c < 8; ++c) out[c] = 0.0f;
    if (!(S.K > 0.0f)) return;
    out[0] = S.A.x / S.K; out[1] = S.A.y / S.K; out[2] = S.A.z / S.K; out[3] = S.K / (float)(n * n);
    out[4] = S.N.x / S.K; out[5] = S.N.y / S.K; out[6] = S.N.z / S.K; out[7] = S.D / S.K;
}

}  // namespace vr
