// vr_temporal.h -- depth-reprojected temporal accumulation in front of the a-trous filter (host + device lane code).
//
// The temporal part of SVGF (Schied et al. 2017): before the spatial filter of vr_denoise.h runs, the current frame is blended with a history
// of the frames before it, fetched where the pixel's first-scatter point lay on the screen of the frame that wrote the history.  Per-pixel
// functions only: the HIP kernels (vr_filters.hip denoise_temporal_kernel; with rejection denoise_temporal_fetch_kernel and
// denoise_temporal_resolve_kernel) and the host builds of the tests (tests/hostkernel/temporal_host.cpp) run the same code, so the two agree bit for bit.  The arithmetic is fixed operation by operation (vr_math.h: -ffp-contract=off, IEEE division,
// sqrt_, floor_); a * b + c below is two roundings unless it is written as one of vr_math.h's dot / mat3_mul / axpy, which are fma chains.
// A participating medium has no surface: the "depth" is the mean first-scatter distance along the pixel's centre ray.
//
// The history, all W x H, row 0 at the bottom: integrated colour C (4 floats) and one record (V, N, K, D): V the integrated variance of the
// mean's luminance, N the number of frames behind the pixel (a float, exact up to 2^24; 0 = none), K and D the coverage and depth of the frame
// that wrote it.  With it goes the camera of that frame (pos', M' = cam_transform, cam_z' as RendererHIP::fill_params forms them).
//
// With "denoise_moments" = 1 the history also carries luminance moments, and V comes from them instead of from v: vr_moments.h.
//
// Pixel (px, py) of the current frame; c = its framebuffer colour, v = denoise_mean_variance of it, (k, d) = coverage and depth of its guide:
//  1 Where it was.  The centre ray is feature_sample's expression with both jitters 0.5:
//      f = (((px + 0.5) - W * 0.5) / H, ((py + 0.5) - H * 0.5) / H, cam_z), dir = normalize(mat3_mul(M, normalize(f)))
//      k > 0: X = axpy(pos, d, dir), r = X - pos', d' = sqrt_(dot(r, r));   k = 0 (environment only): r = dir, d' is not used
//      q = M'^T r: q.x = fma(M'[2], r.z, fma(M'[1], r.y, M'[0] * r.x)), q.y from M'[3..5], q.z from M'[6..8] (M' is a rotation: its transpose
//      inverts it).  q.z >= 0: no history.
//      s = cam_z' / q.z, u = ((q.x * s) * H + W * 0.5) - 0.5, w = ((q.y * s) * H + H * 0.5) - 0.5
//      x0 = floor_(u), y0 = floor_(w), ax = u - x0, ay = w - y0
//  2 Taps.  The four pixels (x0 + dx, y0 + dy), dy outer, dx inner, bilinear weight b = (dx ? ax : 1 - ax) * (dy ? ay : 1 - ay).  A tap counts
//    iff it lies inside the frame (tested before anything is read), b > 0, N_q >= 1 and it shows the same kind of thing:
//      (k > 0 and K_q > 0 and |D_q - d'| <= 0.1 * max_(D_q, d'))  or  (k = 0 and K_q = 0)
//    0.1 is kDenoiseDefaultSigma's depth width used as a hard bound.  Comparisons with NaN are false, so a NaN depth has no history.
//    sum b over the taps that count < 2^-10: no history.  Otherwise h = (sum b C_q) / sum b per channel, v_h = (sum b V_q) / sum b, each sum
//    from 0 in tap order, and N_h = the smallest N_q of the taps that count.
//  2a The pixel against its history (only with a rejection threshold tau > 0, off by default).  A pixel with a history gets the squared z-score
//      dl = luma(h.rgb) - luma(c.rgb), z2 = (dl * dl) / ((v + v_h) + 1e-12)
//    of the two estimates of its luminance: v and v_h are the variances of the two, so z2 has expectation 1 while the scene did not change.
//    luma is vr_math.h's, the division IEEE.  A frame of n = 1 samples has v = 0 and rejects whatever changed at all: the test needs n >= 2.
//    The floor 1e-12 assumes radiances far above 1e-6.
//  3 Unchanged camera.  If pos, M and cam_z equal the history's byte for byte (decided by the caller from what it can see, not an option), step 1
//    is skipped: u = px, w = py, d' = d, so the one tap with b > 0 is (px, py) with b = 1 and h = C_q exactly.  No resampling blur builds up
//    under a fixed camera.
//  3a Rejection (tau > 0 only), at a pixel p with a history: T = (sum z2_q) / count over the pixels q = p + (dx, dy), dx and dy in -2 .. 2, dy outer,
//    dx inner, that lie inside the frame and have a history; the sum from 0, count a float, p itself among them.  The pixel is rejected iff
//    !(T <= tau) -- a NaN rejects -- and is from here on a pixel without history.  One z2 is too noisy to threshold; the mean of up to 25 is not.
//    In the window a pixel stands as one word, its z2 or -1 for "no history or off the frame": variances are >= 0, so no z2 is negative.
//  4 Blend.  No history: C = c, V = v, N = 1.  Otherwise N = min(N_h + 1, 2^20), a = max_(alpha, 1 / N), oma = 1 - a,
//      C = oma * h + a * c per channel, V = (oma * oma) * v_h + (a * a) * v.   (C, V, N, k, d) is the new history.
//  5 The a-trous iterations of vr_denoise.h then run unchanged from (C, V) with the current frame's guide; with 0 iterations the result is C.
//
// The blend treats frames as equals: it is meant for sequences of equal samples per pixel per frame.  Once per frame: a second call on the same
// frame blends the frame with itself.  A reprojected pixel whose u or w is not in [-1, W) x [-1, H) (NaN included) has all four taps off the frame;
// it is "no history" before any index is formed.
#pragma once

#include "vr_math.h"

namespace vr {

struct TemporalCamera { float pos[3]; float m[9]; float cam_z; };      // cam_pos, cam_transform (column-major), cam_z of one frame
constexpr float kTemporalDefaultAlpha = 0.1f;
constexpr float kTemporalAlphaMin = 0x1p-20f, kTemporalAlphaMax = 1.0f;      // the accepted range of "denoise_alpha"
constexpr float kTemporalDepthBound = 0.1f;           // relative depth difference a tap may have (kDenoiseDefaultSigma[2] as a hard bound)
constexpr float kTemporalMinWeight = 0x1p-10f;        // smallest sum of bilinear weights that still is a history
constexpr float kTemporalMaxLength = 1048576.0f;      // 2^20 frames
constexpr float kTemporalRejectMin = 0x1p-10f, kTemporalRejectMax = 0x1p20f;      // the accepted range of "denoise_reject" besides 0 = off
constexpr float kTemporalVarianceFloor = 1e-12f;      // added to the variance of the difference (radiances far above 1e-6)
constexpr int32_t kTemporalWindow = 2;                // the rejection statistic pools a (2 * 2 + 1)^2 window
constexpr float kTemporalNoHistory = -1.0f;           // the statistic, and the window word, of a pixel without a history

// cam_z of the uniform block (common.glsl:78).  Cameras are compared byte for byte (step 3), so there is one expression for it: RendererHIP::fill_params
// and run_denoise call it, and so does the tests' host build.  No kernel does.
VR_HD float camera_z(float fov_degree) { return -0.5f / tan_(0.5f * kPi * fov_degree / 180.f); }

// Step 1: where the first-scatter point of pixel (px, py) lay on the history's screen (u, w in pixels, d' its distance from that camera).
// false: behind that camera (q.z >= 0 or NaN); u, w, d' are not written then.
VR_HD bool temporal_reproject(const TemporalCamera& cur, const TemporalCamera& prev, int32_t W, int32_t H, int32_t px, int32_t py, float k, float d,
                              float& u, float& w, float& dprev) {
    const float fW = (float)W, fH = (float)H;
    const float fx = (((float)px + 0.5f) - fW * 0.5f) / fH;
    const float fy = (((float)py + 0.5f) - fH * 0.5f) / fH;
    const v3 dir = normalize(mat3_mul(cur.m, normalize(v3{ fx, fy, cur.cam_z })));
    v3 r = dir;
    float dp = 0.0f;
    if (k > 0.0f) {
        const v3 X = axpy(v3{ cur.pos[0], cur.pos[1], cur.pos[2] }, d, dir);
        r = X - v3{ prev.pos[0], prev.pos[1], prev.pos[2] };
        dp = sqrt_(dot(r, r));
    }
    const v3 q = v3{ fma_(prev.m[2], r.z, fma_(prev.m[1], r.y, prev.m[0] * r.x)),
                     fma_(prev.m[5], r.z, fma_(prev.m[4], r.y, prev.m[3] * r.x)),
                     fma_(prev.m[8], r.z, fma_(prev.m[7], r.y, prev.m[6] * r.x)) };
    if (!(q.z < 0.0f)) return false;
    const float s = prev.cam_z / q.z;
    u = ((q.x * s) * fH + fW * 0.5f) - 0.5f;
    w = ((q.y * s) * fH + fH * 0.5f) - 0.5f;
    dprev = dp;
    return true;
}

// Steps 1-3 at pixel (px, py): the fetch.  Hist reads the previous history by pixel index y * W + x:
//   void color(int32_t i, float c[4]) const;   void record(int32_t i, float s[4]) const;      (V, N, K, D)
// have: a history exists; same_cam: its camera equals the current one byte for byte.  true: the pixel has a history, h, vh, nh are step 2's
// h, v_h, N_h; false: they are 0.  extra.tap(iq, b) is called for every tap that counts, in tap order, with its pixel index and bilinear weight: what
// else the history carries per pixel is gathered from the same taps (vr_moments.h).
struct TemporalNoExtra { VR_HD void tap(int32_t, float) {} };
template <class Hist, class Extra>
VR_HD bool temporal_fetch(const Hist& hist, bool have, bool same_cam, const TemporalCamera& cur, const TemporalCamera& prev, int32_t W, int32_t H,
                          int32_t px, int32_t py, float k, float d, float h[4], float& vh, float& nh_out, Extra& extra) {
    float hs[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    float bs = 0.0f, vs = 0.0f, nh = 0.0f;
    bool any = false;
    float u = (float)px, w = (float)py, dp = d;
    bool on = have;
    if (on && !same_cam) on = temporal_reproject(cur, prev, W, H, px, py, k, d, u, w, dp);
    if (on && u >= -1.0f && u < (float)W && w >= -1.0f && w < (float)H) {
        const float fx0 = floor_(u), fy0 = floor_(w);
        const float ax = u - fx0, ay = w - fy0;
        const int32_t x0 = (int32_t)fx0, y0 = (int32_t)fy0;
        for (int32_t dy = 0; dy <= 1; ++dy) {
            const int32_t y = y0 + dy;
            if (y < 0 || y >= H) continue;
            for (int32_t dx = 0; dx <= 1; ++dx) {
                const int32_t x = x0 + dx;
                if (x < 0 || x >= W) continue;
                const float b = (dx ? ax : 1.0f - ax) * (dy ? ay : 1.0f - ay);
                if (!(b > 0.0f)) continue;
                const int32_t iq = y * W + x;
                float s[4];
                hist.record(iq, s);
                if (!(s[1] >= 1.0f)) continue;
                const bool same = k > 0.0f ? (s[2] > 0.0f && abs_(s[3] - dp) <= kTemporalDepthBound * max_(s[3], dp)) : (k == 0.0f && s[2] == 0.0f);
                if (!same) continue;
                float cq[4];
                hist.color(iq, cq);
                for (int32_t i = 0; i < 4; ++i) hs[i] = hs[i] + b * cq[i];
                vs = vs + b * s[0];
                bs = bs + b;
                nh = any ? min_(nh, s[1]) : s[1];
                any = true;
                extra.tap(iq, b);
            }
        }
    }
    if (!any || bs < kTemporalMinWeight) {
        for (int32_t i = 0; i < 4; ++i) h[i] = 0.0f;
        vh = 0.0f; nh_out = 0.0f;
        return false;
    }
    for (int32_t i = 0; i < 4; ++i) h[i] = hs[i] / bs;
    vh = vs / bs;
    nh_out = nh;
    return true;
}
template <class Hist>
VR_HD bool temporal_fetch(const Hist& hist, bool have, bool same_cam, const TemporalCamera& cur, const TemporalCamera& prev, int32_t W, int32_t H,
                          int32_t px, int32_t py, float k, float d, float h[4], float& vh, float& nh_out) {
    TemporalNoExtra none;
    return temporal_fetch(hist, have, same_cam, cur, prev, W, H, px, py, k, d, h, vh, nh_out, none);
}

// Step 4 at a pixel: keep = the pixel has a history and it was not rejected; (h, vh, nh) its fetch.  Cout / Sout: the pixel's new history.
VR_HD void temporal_blend(bool keep, const float h[4], float vh, float nh, const float c[4], float v, float k, float d, float alpha, float Cout[4],
                          float Sout[4]) {
    Sout[2] = k; Sout[3] = d;
    if (!keep) {
        for (int32_t i = 0; i < 4; ++i) Cout[i] = c[i];
        Sout[0] = v; Sout[1] = 1.0f;
        return;
    }
    const float N = min_(nh + 1.0f, kTemporalMaxLength);
    const float a = max_(alpha, 1.0f / N), oma = 1.0f - a;
    for (int32_t i = 0; i < 4; ++i) Cout[i] = oma * h[i] + a * c[i];
    Sout[0] = (oma * oma) * vh + (a * a) * v;
    Sout[1] = N;
}

// Steps 1-4 at pixel (px, py), without the rejection test: the fetch, then the blend.
template <class Hist>
VR_HD void temporal_pixel(const Hist& hist, bool have, bool same_cam, const TemporalCamera& cur, const TemporalCamera& prev, int32_t W, int32_t H,
                          int32_t px, int32_t py, const float c[4], float v, float k, float d, float alpha, float Cout[4], float Sout[4]) {
    float h[4], vh, nh;
    const bool has = temporal_fetch(hist, have, same_cam, cur, prev, W, H, px, py, k, d, h, vh, nh);
    temporal_blend(has, h, vh, nh, c, v, k, d, alpha, Cout, Sout);
}

// Step 2a at a pixel with a history: the squared z-score of its fetch against the frame.
VR_HD float temporal_z2(const float h[4], float vh, const float c[4], float v) {
    const float dl = luma(v3{ h[0], h[1], h[2] }) - luma(v3{ c[0], c[1], c[2] });
    return (dl * dl) / ((v + vh) + kTemporalVarianceFloor);
}
// the word that stands for a pixel in step 3a's window: its z2, or kTemporalNoHistory (the only negative one, variances being >= 0) without a history
VR_HD float temporal_window_word(bool has, float z2) { return has ? z2 : kTemporalNoHistory; }
// Step 3a at a pixel with a history.  Win answers  float word(int32_t dx, int32_t dy) const:  the window word of pixel p + (dx, dy),
// kTemporalNoHistory where that pixel lies outside the frame.  A NaN word counts, and makes T NaN.
template <class Win>
VR_HD float temporal_pool(const Win& win) {
    float sum = 0.0f, count = 0.0f;
    for (int32_t dy = -kTemporalWindow; dy <= kTemporalWindow; ++dy)
        for (int32_t dx = -kTemporalWindow; dx <= kTemporalWindow; ++dx) {
            const float z = win.word(dx, dy);
            if (z < 0.0f) continue;
            sum = sum + z;
            count = count + 1.0f;
        }
    return sum / count;
}
VR_HD bool temporal_rejects(float T, float tau) { return !(T <= tau); }

}  // namespace vr
