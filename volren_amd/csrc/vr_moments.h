// vr_moments.h -- temporal luminance moments: the variance that drives the a-trous filter, taken from the history (host + device lane code).
//
// The variance estimate of SVGF (Schied et al. 2017, section 4.2).  vr_denoise.h's filter is driven by the per-pixel sample variance of the frame, which
// a frame of one sample per pixel does not have.  With "denoise_moments" = 1 the temporal accumulation of vr_temporal.h carries, per pixel, the
// integrated first and second moments of the frame's luminance, and the variance of the filter's input comes from them: temporally where the history
// is long enough, from a guide-weighted 7 x 7 neighbourhood where it is not (the first frames, disoccluded pixels).  Per-pixel functions only: the HIP
// kernels (vr_filters.hip denoise_temporal_kernel<true>, denoise_moments_variance_kernel) and the host build of the tests
// (tests/hostkernel/moments_host.cpp) run the same code, so the two agree bit for bit.  The arithmetic is fixed operation by operation (vr_math.h:
// -ffp-contract=off, IEEE division, luma, max_, exp_, pow_, sqrt_); a * b + c below is two roundings.
//
// The history gains a third array beside vr_temporal.h's colour and record: the moment record (m1, m2, E, S), W x H float4, row 0 at the bottom.
//   m1, m2  the integrated first and second moments of L = luma(c.rgb), c the frame's colour
//   E       the sum of squared blend weights behind the pixel: the variance of the integrated luminance is E times that of one frame's
//   S       the variance of one frame's luminance, as estimated by the call that wrote the record
//
// Pass 1, pixel p (with vr_temporal.h's steps 1-4, which stay what they are for C, N, K, D):
//   Fetch.  The taps that count in step 2, in the same order, with the same weights b, also give
//     m1_h = (sum b m1_q) / sum b,  m2_h = (sum b m2_q) / sum b,  E_h = (sum b E_q) / sum b,        each sum from 0, sum b too (it is step 2's, bit for bit)
//   Blend.  L = luma(c.rgb).  No history: m1 = L, m2 = L * L, E = 1.  Otherwise, with step 4's N, a = max_(alpha, 1 / N), oma = 1 - a:
//     m1 = oma * m1_h + a * L,  m2 = oma * m2_h + a * (L * L),  E = (oma * oma) * E_h + a * a
//   The frame's own v is not used: pass 1 blends V from v = v_h = 0, and pass 2 overwrites it.  S = 0 until pass 2.
// Pass 2, pixel p, after pass 1 of every pixel (it reads the neighbours' m1, m2); N_p the pixel's new length:
//   N_p >= kMomentsMinLength (4):  S = max_(m2 - m1 * m1, 0)
//   otherwise (a NaN length included) the moments are pooled over q = p + (dx, dy), dx, dy in -3 .. 3, dy outer, dx inner, taps outside the frame skipped:
//     w = 1 at the centre tap, exactly; elsewhere w = w_k, and where k_p > 0 and k_q > 0: w = ((w_k * w_n) * w_d) * w_a -- vr_denoise.h's four guide
//     factors, expression for expression, with the current "denoise_sigma" and the current frame's guide; no luminance factor, no B3 factor
//     a1 = (sum w m1_q) / sum w,  a2 = (sum w m2_q) / sum w,  each sum from 0;  S = max_(a2 - a1 * a1, 0)
//   V = S * E.  V goes into the record's V word and over the pixel's v, where the iterations of vr_denoise.h read it; S into the moment record.
// The iterations then run unchanged from (C, V).  On the first call of a sequence N = 1 everywhere, so every pixel pools: a single 1-spp frame is filtered.
//
// NaN and the rest.  Nothing is sanitised.  A NaN colour makes L, m1, m2 NaN at its pixel; max_(NaN, 0) is NaN (vr_math.h: x < y ? y : x), so S and V
// are NaN there and at every pixel with N < 4 whose window holds it (w * NaN is NaN even for w = 0), and the filter does with a NaN variance what it does
// today.  m2 is a sum of squares under non-negative weights: never negative.  That frees -1 to stand for "off the frame" in a staged window (kMomentsOffFrame),
// tested as m2 < 0, which a NaN fails.  E lies in (0, 1]; a record written by pass 1 alone is never read: the two passes are one call.
// A pass-2 thread writes only words of its own pixel that no neighbour reads (S, V, v); neighbours read m1, m2 only.
#pragma once

#include "vr_denoise.h"
#include "vr_temporal.h"

namespace vr {

constexpr float kMomentsMinLength = 4.0f;             // history length from which the temporal variance is trusted (SVGF)
constexpr int32_t kMomentsWindow = 3;                 // the spatial estimate pools a (2 * 3 + 1)^2 window (SVGF)
constexpr float kMomentsOffFrame = -1.0f;             // the m2 word of a window pixel that lies outside the frame

// The fetch's share: temporal_fetch calls tap(iq, b) for every tap that counts, in order.  Mom reads the previous moment records by pixel index:
//   void moments(int32_t i, float m[4]) const;      (m1, m2, E, S)
template <class Mom>
struct MomentsTaps {
    const Mom& mom;
    float sb = 0.0f, s1 = 0.0f, s2 = 0.0f, sE = 0.0f;
    VR_HD void tap(int32_t iq, float b) {
        float m[4];
        mom.moments(iq, m);
        s1 = s1 + b * m[0];
        s2 = s2 + b * m[1];
        sE = sE + b * m[2];
        sb = sb + b;
    }
};

// Pass 1's blend at a pixel: keep = the pixel has a history; (m1h, m2h, Eh, nh) its fetch.  M: the pixel's new moment record, S = 0.
VR_HD void moments_blend(bool keep, float m1h, float m2h, float Eh, float nh, const float c[4], float alpha, float M[4]) {
    const float L = luma(v3{ c[0], c[1], c[2] });
    M[3] = 0.0f;
    if (!keep) {
        M[0] = L; M[1] = L * L; M[2] = 1.0f;
        return;
    }
    const float N = min_(nh + 1.0f, kTemporalMaxLength);
    const float a = max_(alpha, 1.0f / N), oma = 1.0f - a;
    M[0] = oma * m1h + a * L;
    M[1] = oma * m2h + a * (L * L);
    M[2] = (oma * oma) * Eh + a * a;
}

// Pass 1 at pixel (px, py): vr_temporal.h's steps 1-4 and the moments with them.  Cout / Sout / Mout: the pixel's new history (V = 0 until pass 2).
template <class Hist, class Mom>
VR_HD void moments_pixel(const Hist& hist, const Mom& mom, bool have, bool same_cam, const TemporalCamera& cur, const TemporalCamera& prev, int32_t W, int32_t H,
                         int32_t px, int32_t py, const float c[4], float k, float d, float alpha, float Cout[4], float Sout[4], float Mout[4]) {
    float h[4], vh, nh;
    MomentsTaps<Mom> taps{ mom };
    const bool has = temporal_fetch(hist, have, same_cam, cur, prev, W, H, px, py, k, d, h, vh, nh, taps);
    temporal_blend(has, h, 0.0f, nh, c, 0.0f, k, d, alpha, Cout, Sout);
    // (has: at least one tap counted and sum b >= 2^-10, so the divisions are by a positive number)
    moments_blend(has, has ? taps.s1 / taps.sb : 0.0f, has ? taps.s2 / taps.sb : 0.0f, has ? taps.sE / taps.sb : 0.0f, nh, c, alpha, Mout);
}

// Pass 2 at pixel (px, py) of length N: S.  Win answers  void moments(int32_t dx, int32_t dy, float m[2]) const:  (m1, m2) of pixel p + (dx, dy),
// m2 = kMomentsOffFrame where that pixel lies outside the frame (asked for every dx, dy in -3 .. 3).  Gd reads the current guide by pixel index
// y * W + x, only of pixels inside the frame:  void guide(int32_t i, float g[8]) const  (vr_denoise.h's Src).
template <class Win, class Gd>
VR_HD float moments_variance(const Win& win, const Gd& gd, int32_t W, int32_t px, int32_t py, float N, const DenoiseSigma& sg) {
    float m[2];
    if (N >= kMomentsMinLength) {
        win.moments(0, 0, m);
        return max_(m[1] - m[0] * m[0], 0.0f);
    }
    float gp[8];
    gd.guide(py * W + px, gp);
    const float sa2 = sg.a * sg.a;
    const v3 np = v3{ gp[4], gp[5], gp[6] }, ap = v3{ gp[0], gp[1], gp[2] };
    const bool np0 = np.x == 0.0f && np.y == 0.0f && np.z == 0.0f;
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int32_t dy = -kMomentsWindow; dy <= kMomentsWindow; ++dy)
        for (int32_t dx = -kMomentsWindow; dx <= kMomentsWindow; ++dx) {
            win.moments(dx, dy, m);
            if (m[1] < 0.0f) continue;                    // off the frame: nothing else of that pixel is touched
            float w = 1.0f;
            if (dx != 0 || dy != 0) {
                float gq[8];
                gd.guide((py + dy) * W + (px + dx), gq);
                w = exp_(-abs_(gp[3] - gq[3]) / sg.k);
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
            s1 = s1 + w * m[0];
            s2 = s2 + w * m[1];
            sw = sw + w;
        }
    const float a1 = s1 / sw, a2 = s2 / sw;
    return max_(a2 - a1 * a1, 0.0f);
}

}  // namespace vr
