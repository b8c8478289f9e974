// tests/hostkernel/moments_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The temporal luminance moments of the lane code (volren_amd/csrc/vr_moments.h) compiled for the host, in the two passes the HIP kernels make:
// hk_moments_pass1 as vr_filters.hip denoise_temporal_kernel<true> (vr_temporal.h's fetch and blend with the moment records), hk_moments_pass2 as
// denoise_moments_variance_kernel (S, V = S * E).  tests/test_moments_host.py checks it against a float64 numpy statement of the rules
// (tests/hk_moments.py); tests/test_gpu_moments.py checks the HIP kernels against it bit for bit.
// A camera is 13 floats: cam_pos (3), cam_transform (9, column-major), cam_z.  checked != 0: every read of the history, of the window and of the
// guide goes through a range check, and the functions return the number of reads outside the frame (0 is the only right answer).
#include <cstdint>

#include "../../volren_amd/csrc/vr_moments.h"
#include "host_frame.h"

using namespace vr;

namespace {
// the window of pixel (px, py) over the whole frame's moment records (the kernel's LDS footprint holds the same pairs)
struct HostWindow {
    const float* m;
    int32_t W, H, px, py;
    Range range;
    void moments(int32_t dx, int32_t dy, float o[2]) const {
        const int32_t x = px + dx, y = py + dy;
        o[0] = 0.0f; o[1] = kMomentsOffFrame;
        if (x < 0 || x >= W || y < 0 || y >= H) return;
        const int64_t i = (int64_t)y * W + x;
        if (!range.ok(i)) return;
        o[0] = m[4 * i]; o[1] = m[4 * i + 1];
    }
};
}  // namespace

extern "C" {

// out = (history length from which the temporal variance counts, window radius, the m2 word of a pixel off the frame)
void hk_moments_constants(float* out) { out[0] = kMomentsMinLength; out[1] = (float)kMomentsWindow; out[2] = kMomentsOffFrame; }

// pass 1 of a whole frame: color W*H*4, k / d W*H, the history (hist_color, hist_record, hist_moments W*H*4; read only if have) -> the new history
// with V = 0 and S = 0
int64_t hk_moments_pass1(int checked, int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* k, const float* d,
                         const float* hist_color, const float* hist_record, const float* hist_moments, float alpha, float* out_color, float* out_record,
                         float* out_moments) {
    int64_t bad = 0;
    const Range range{ (int64_t)W * H, checked ? &bad : nullptr };
    const TemporalCamera cc = camera_of(cur), pc = camera_of(prev);
    const HostHist hist{ hist_color, hist_record, range };
    const HostMoments mom{ hist_moments, range };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            moments_pixel(hist, mom, have != 0, same_cam != 0, cc, pc, W, H, x, y, color + 4 * i, k[i], d[i], alpha, out_color + 4 * i, out_record + 4 * i,
                          out_moments + 4 * i);
        }
    return bad;
}

// pass 2 of a whole frame, in place on pass 1's record and moments: guide W*H*8, sigma 5 floats (vr_denoise.h's order) -> S into the moment records,
// V = S * E into the records and into v (W*H)
int64_t hk_moments_pass2(int checked, int W, int H, const float* guide, const float* sigma, float* record, float* moments, float* v) {
    int64_t bad = 0;
    const Range range{ (int64_t)W * H, checked ? &bad : nullptr };
    const DenoiseSigma sg{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] };
    const HostGuide gd{ guide, range };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            const float S = moments_variance(HostWindow{ moments, W, H, x, y, range }, gd, W, x, y, record[4 * i + 1], sg);
            const float V = S * moments[4 * i + 2];
            moments[4 * i + 3] = S;      // (neighbours read m1, m2 only: in place is what the kernel does)
            record[4 * i] = V;
            v[i] = V;
        }
    return bad;
}

}
