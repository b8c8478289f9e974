// tests/hostkernel/temporal_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The temporal accumulation of the lane code (volren_amd/csrc/vr_temporal.h) compiled for the host, without its history rejection (hk_temporal_*: one
// pass, as vr_filters.hip denoise_temporal_kernel) and with it (hk_reject_*: steps 2a and 3a, in the two passes of denoise_temporal_fetch_kernel and
// denoise_temporal_resolve_kernel).  tests/test_temporal_host.py and tests/test_reject_host.py check it against a float64 numpy statement of the rules
// (tests/hk_temporal.py); tests/test_gpu_temporal.py and tests/test_gpu_reject.py check the HIP kernels against it bit for bit.
// A camera is 13 floats: cam_pos (3), cam_transform (9, column-major), cam_z.
#include <cstdint>
#include <vector>

#include "../../volren_amd/csrc/vr_temporal.h"
#include "host_frame.h"

using namespace vr;

namespace {
// every read of the history (host_frame.h HostHist) and of the window goes through a Range
// the window of pixel (px, py) over the whole frame's z2 / has planes (the kernel's LDS footprint holds the same words)
struct HostWindow {
    const float* z2;
    const uint8_t* has;
    int32_t W, H, px, py;
    Range range;
    float word(int32_t dx, int32_t dy) const {
        const int32_t x = px + dx, y = py + dy;
        if (x < 0 || x >= W || y < 0 || y >= H) return kTemporalNoHistory;
        const int64_t i = (int64_t)y * W + x;
        if (!range.ok(i)) return kTemporalNoHistory;
        return temporal_window_word(has[i] != 0, z2[i]);
    }
};
// steps 1-4 of a whole frame; out_stat = nullptr: without 2a and 3a, in one pass.  -> the number of reads outside the frame (counted only if checked)
int64_t step_frame(bool checked, int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k,
                   const float* d, const float* hist_color, const float* hist_record, float alpha, float tau, float* out_color, float* out_record, float* out_stat) {
    int64_t bad = 0;
    const Range range{ (int64_t)W * H, checked ? &bad : nullptr };
    const TemporalCamera cc = camera_of(cur), pc = camera_of(prev);
    const size_t n = (size_t)W * H;
    const HostHist hist{ hist_color, hist_record, range };
    if (!out_stat) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                temporal_pixel(hist, have != 0, same_cam != 0, cc, pc, W, H, x, y, color + 4 * i, v[i], k[i], d[i], alpha, out_color + 4 * i, out_record + 4 * i);
            }
        return bad;
    }
    std::vector<float> h(4 * n), vh(n), nh(n), z2(n);
    std::vector<uint8_t> has(n);
    for (int y = 0; y < H; ++y)                           // the fetch
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            has[i] = temporal_fetch(hist, have != 0, same_cam != 0, cc, pc, W, H, x, y, k[i], d[i], &h[4 * i], vh[i], nh[i]) ? 1 : 0;
            z2[i] = has[i] ? temporal_z2(&h[4 * i], vh[i], color + 4 * i, v[i]) : 0.0f;
        }
    for (int y = 0; y < H; ++y)                           // the resolve
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            float T = kTemporalNoHistory;
            if (has[i]) T = temporal_pool(HostWindow{ z2.data(), has.data(), W, H, x, y, range });
            temporal_blend(has[i] && !temporal_rejects(T, tau), &h[4 * i], vh[i], nh[i], color + 4 * i, v[i], k[i], d[i], alpha, out_color + 4 * i, out_record + 4 * i);
            out_stat[i] = T;
        }
    return bad;
}
}  // namespace

extern "C" {

// cam_z of a field of view in degrees: the renderer's own expression
float hk_temporal_cam_z(float fov_degree) { return camera_z(fov_degree); }

// out = (default alpha, smallest alpha, largest alpha, depth bound, smallest weight sum, longest history)
void hk_temporal_constants(float* out) {
    out[0] = kTemporalDefaultAlpha; out[1] = kTemporalAlphaMin; out[2] = kTemporalAlphaMax;
    out[3] = kTemporalDepthBound; out[4] = kTemporalMinWeight; out[5] = kTemporalMaxLength;
}
// out = (smallest tau, largest tau, variance floor, window radius, the statistic of a pixel without history)
void hk_reject_constants(float* out) {
    out[0] = kTemporalRejectMin; out[1] = kTemporalRejectMax; out[2] = kTemporalVarianceFloor; out[3] = (float)kTemporalWindow; out[4] = kTemporalNoHistory;
}

// step 1 alone: k, d = W*H coverage and depth -> u, w, dprev (W*H each; untouched where ok = 0), ok (W*H: in front of the history's camera)
void hk_temporal_reproject(int W, int H, const float* cur, const float* prev, const float* k, const float* d, float* u, float* w, float* dprev, int32_t* ok) {
    const TemporalCamera cc = camera_of(cur), pc = camera_of(prev);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            ok[i] = temporal_reproject(cc, pc, W, H, x, y, k[i], d[i], u[i], w[i], dprev[i]) ? 1 : 0;
        }
}

// steps 1-4 of a whole frame: color W*H*4, v / k / d W*H, the history (hist_color, hist_record W*H*4; read only if have) -> the new history
void hk_temporal_step(int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k,
                      const float* d, const float* hist_color, const float* hist_record, float alpha, float* out_color, float* out_record) {
    step_frame(false, W, H, have, same_cam, cur, prev, color, v, k, d, hist_color, hist_record, alpha, 0.0f, out_color, out_record, nullptr);
}
// the same with every history read behind a range check: returns the number of reads outside the frame (0 is the only right answer)
int64_t hk_temporal_step_checked(int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k,
                                 const float* d, const float* hist_color, const float* hist_record, float alpha, float* out_color, float* out_record) {
    return step_frame(true, W, H, have, same_cam, cur, prev, color, v, k, d, hist_color, hist_record, alpha, 0.0f, out_color, out_record, nullptr);
}

// steps 1-4 with 2a and 3a, tau > 0: as hk_temporal_step, and the statistic T (W*H; -1 without history)
void hk_reject_step(int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k, const float* d,
                    const float* hist_color, const float* hist_record, float alpha, float tau, float* out_color, float* out_record, float* out_stat) {
    step_frame(false, W, H, have, same_cam, cur, prev, color, v, k, d, hist_color, hist_record, alpha, tau, out_color, out_record, out_stat);
}
// the same with every history and window read behind a range check
int64_t hk_reject_step_checked(int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k,
                               const float* d, const float* hist_color, const float* hist_record, float alpha, float tau, float* out_color, float* out_record,
                               float* out_stat) {
    return step_frame(true, W, H, have, same_cam, cur, prev, color, v, k, d, hist_color, hist_record, alpha, tau, out_color, out_record, out_stat);
}

}
