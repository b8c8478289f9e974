// tests/hostkernel/temporal_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The temporal accumulation of the lane code (volren_amd/csrc/vr_temporal.h) compiled for the host: tests/test_temporal_host.py checks it against a
// float64 numpy statement of the rules (tests/hk_temporal.py), and tests/test_gpu_temporal.py checks the HIP kernel against it bit for bit.
// A camera is 13 floats: cam_pos (3), cam_transform (9, column-major), cam_z.
#include <cstdint>
#include <cstring>

#include "../../volren_amd/csrc/vr_temporal.h"

using namespace vr;

namespace {
struct HostHist {
    const float* c;      // W*H*4
    const float* s;      // W*H*4: (V, N, K, D)
    void color(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = c[4 * (size_t)i + k]; }
    void record(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = s[4 * (size_t)i + k]; }
};
// the same reads behind a range check: an index outside [0, n) is counted and answered with zeros, never dereferenced
struct CheckedHist {
    HostHist h;
    int64_t n;
    int64_t* bad;
    void color(int32_t i, float o[4]) const { if (i < 0 || i >= n) { ++*bad; for (int k = 0; k < 4; ++k) o[k] = 0.0f; } else h.color(i, o); }
    void record(int32_t i, float o[4]) const { if (i < 0 || i >= n) { ++*bad; for (int k = 0; k < 4; ++k) o[k] = 0.0f; } else h.record(i, o); }
};
TemporalCamera camera_of(const float* p) {
    TemporalCamera c;
    std::memcpy(c.pos, p, 3 * sizeof(float));
    std::memcpy(c.m, p + 3, 9 * sizeof(float));
    c.cam_z = p[12];
    return c;
}
template <class Hist>
void step_frame(const Hist& hist, int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k,
                const float* d, float alpha, float* out_color, float* out_record) {
    const TemporalCamera cc = camera_of(cur), pc = camera_of(prev);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)y * W + x;
            temporal_pixel(hist, have != 0, same_cam != 0, cc, pc, W, H, x, y, color + 4 * i, v[i], k[i], d[i], alpha, out_color + 4 * i, out_record + 4 * i);
        }
}
}  // namespace

extern "C" {

// cam_z of a field of view in degrees, as RendererHIP::fill_params forms it
float hk_temporal_cam_z(float fov_degree) { return -0.5f / tan_(0.5f * kPi * fov_degree / 180.f); }

// out = (default alpha, smallest alpha, largest alpha, depth bound, smallest weight sum, longest history)
void hk_temporal_constants(float* out) {
    out[0] = kTemporalDefaultAlpha; out[1] = kTemporalAlphaMin; out[2] = kTemporalAlphaMax;
    out[3] = kTemporalDepthBound; out[4] = kTemporalMinWeight; out[5] = kTemporalMaxLength;
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
    step_frame(HostHist{ hist_color, hist_record }, W, H, have, same_cam, cur, prev, color, v, k, d, alpha, out_color, out_record);
}

// the same through CheckedHist: returns the number of history reads outside the frame (0 is the only right answer)
int64_t hk_temporal_step_checked(int W, int H, int have, int same_cam, const float* cur, const float* prev, const float* color, const float* v, const float* k,
                                 const float* d, const float* hist_color, const float* hist_record, float alpha, float* out_color, float* out_record) {
    int64_t bad = 0;
    step_frame(CheckedHist{ HostHist{ hist_color, hist_record }, (int64_t)W * H, &bad }, W, H, have, same_cam, cur, prev, color, v, k, d, alpha, out_color, out_record);
    return bad;
}

}
