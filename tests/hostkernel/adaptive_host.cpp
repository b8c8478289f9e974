// tests/hostkernel/adaptive_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The adaptive-sampling lane code (volren_amd/csrc/vr_adaptive.h) compiled for the host: tests/test_adaptive_host.py checks it against a float64
// numpy statement (tests/hk_adaptive.py), and tests/test_gpu_adaptive.py checks the error kernel and the renderer's schedule against it bit for bit.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../volren_amd/csrc/vr_adaptive.h"

using namespace vr;

namespace {
struct HostSrc {
    const float* c;      // W*H*4
    const float* v;      // W*H
    const float* g;      // W*H*8
    void color(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = c[4 * (size_t)i + k]; }
    float var(int32_t i) const { return v[i]; }
    void guide(int32_t i, float o[8]) const { for (int k = 0; k < 8; ++k) o[k] = g[8 * (size_t)i + k]; }
};
}  // namespace

extern "C" {

// e_p of every pixel: mu, S = W*H*4 (framebuffer, moments), n = W*H counts -> e (W*H)
void hk_adaptive_pixel_error(int n_px, const float* mu, const float* S, const int32_t* n, float* e) {
    for (int i = 0; i < n_px; ++i) e[i] = adaptive_pixel_error(mu + 4 * (size_t)i, S + 4 * (size_t)i, n[i]);
}

// e_t of every raster tile of a W x H frame, tile t holding counts[t] samples (row 0 = bottom, pixels in raster order).  from_var: `S` holds the
// unbiased variance as vr_variance returns it (S * n / (n - 1), 0 for n < 2: the same bits the kernel forms from the moments)
void hk_adaptive_tile_error(int W, int H, const float* mu, const float* S, const int32_t* counts, int from_var, float* e_t) {
    const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
    for (int t = 0; t < tiles_x * tiles_y; ++t) e_t[t] = -inf_();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int t = (y / 16) * tiles_x + x / 16;
            const size_t i = (size_t)y * W + x;
            const float e = !from_var ? adaptive_pixel_error(mu + 4 * i, S + 4 * i, counts[t])
                                      : (counts[t] < 2 ? inf_() : adaptive_error_of_variance(mu + 4 * i, S + 4 * i, counts[t]));
            e_t[t] = adaptive_max(e_t[t], e);
        }
}

int hk_adaptive_next_count(int n, int max_spp) { return adaptive_next_count(n, max_spp); }
int hk_adaptive_converged(float e, float threshold) { return adaptive_converged(e, threshold) ? 1 : 0; }
float hk_adaptive_floor(void) { return kAdaptiveFloor; }

// adaptive_groups of ids (counts by raster tile id): out_n[g], out_len[g] per group, out_tiles = the groups one after another; returns the group count
int hk_adaptive_groups(const int32_t* ids, int n_ids, const int32_t* counts, int n_counts, int32_t* out_n, int32_t* out_len, int32_t* out_tiles) {
    const auto g = adaptive_groups(std::vector<int32_t>(ids, ids + n_ids), std::vector<int32_t>(counts, counts + n_counts));
    int k = 0;
    size_t off = 0;
    for (const auto& e : g) {
        out_n[k] = e.first;
        out_len[k] = (int32_t)e.second.size();
        std::memcpy(out_tiles + off, e.second.data(), e.second.size() * sizeof(int32_t));
        off += e.second.size();
        ++k;
    }
    return k;
}

// denoise_prepare_kernel with per-pixel counts (a ragged frame): var = W*H*4 unbiased variances as vr_variance gives them (each tile's own factor,
// the kernel's formation), n = W*H counts -> v (W*H), guide (W*H*8)
void hk_adaptive_denoise_prepare(int W, int H, const int32_t* n, const float* var, const float* feat, float* v, float* guide) {
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        v[i] = denoise_mean_variance(var + 4 * i, n[i]);
        denoise_guide(feat + 8 * i, guide + 8 * i);
    }
}

// the whole denoiser of a ragged frame: prepare with per-pixel n, then N a-trous iterations at steps 1, 2, 4, ...
void hk_adaptive_denoise(int W, int H, const int32_t* n, const float* color, const float* var, const float* feat, int N, const float* sigma, float* out) {
    const size_t px = (size_t)W * H;
    std::vector<float> v(px), v2(px), g(8 * px), c(color, color + 4 * px), c2(4 * px);
    hk_adaptive_denoise_prepare(W, H, n, var, feat, v.data(), g.data());
    const DenoiseSigma sg{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] };
    for (int k = 0; k < N; ++k) {
        const HostSrc src{ c.data(), v.data(), g.data() };
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)y * W + x;
                denoise_atrous_pixel(src, W, H, x, y, 1 << k, sg, c2.data() + 4 * i, v2[i]);
            }
        c.swap(c2);
        v.swap(v2);
    }
    std::memcpy(out, c.data(), 4 * px * sizeof(float));
}

}
