// tests/hostkernel/upsample_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The upsampling of the scattered layer (volren_amd/csrc/vr_upsample.h) compiled for the host, with the window of a hi tile in the lo frame that its kernel stages
// (volren_amd/csrc/vr_tiles.h ScaledTileWindow): tests/test_upsample_host.py checks them against a float64 statement of the header and statements of the
// window (tests/hk_upsample.py), and tests/test_gpu_upsample.py checks the HIP kernel against this build.
#include <stddef.h>
#include <stdint.h>

#include "../../volren_amd/csrc/vr_tiles.h"
#include "../../volren_amd/csrc/vr_upsample.h"

using namespace vr;

namespace {
struct HostTaps {
    const float* L;        // w*h*4
    const float* g;        // w*h*8
    int32_t w;
    void tap(int32_t lx, int32_t ly, float Lq[4], float gq[8]) const {
        const size_t i = (size_t)ly * w + lx;
        for (int c = 0; c < 4; ++c) Lq[c] = L[4 * i + c];
        for (int c = 0; c < 8; ++c) gq[c] = g[8 * i + c];
    }
};

template <int32_t F>
int window_of(int tile, int W, int32_t* geom, int32_t* at) {
    const ScaledTileWindow<F> window = ScaledTileWindow<F>::of(tile, W);
    geom[0] = window.kFoot; geom[1] = window.kTexels; geom[2] = window.x0; geom[3] = window.y0;
    for (uint32_t t = 0; t < 256u; ++t) {
        const TilePixel q = wave_tiled_pixel(tile, t, W);
        int32_t x0, y0, r;
        upsample_split(q.px, F, x0, r);
        upsample_split(q.py, F, y0, r);
        at[t] = window.at(x0 - 1, y0 - 1);       // the first of the pixel's 4 x 4 taps; tap (i, j) lies j * kFoot + i further on
    }
    return 0;
}
}

extern "C" {

// the guide of n pixels' features: n*8 -> n*8
void hk_upsample_guide(int n, const float* feat, float* g) {
    for (size_t p = 0; p < (size_t)n; ++p) denoise_guide(feat + 8 * p, g + 8 * p);
}

// The whole hi frame.  L = w*h*4 the lo layer, glo = w*h*8 the lo guide, ghi = W*H*8 the hi guide, B = W*H*4 the hi background, sigma = the five of
// "denoise_sigma" -> out, Lout = W*H*4 each, W = f w, H = f h, row 0 at the bottom
void hk_upsample(int w, int h, int f, const float* L, const float* glo, const float* ghi, const float* B, const float* sigma, float* out, float* Lout) {
    const DenoiseSigma sg{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] };
    const int W = f * w, H = f * h;
    const HostTaps src{ L, glo, w };
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        upsample_pixel(src, w, h, f, x, y, ghi + 8 * p, B + 4 * p, sg, Lout + 4 * p, out + 4 * p);
    }
}

// per axis: xr = (x0, r) of hi coordinate x, a = the fraction as the lane code forms it, b = the spline's four weights at it
void hk_upsample_axis(int x, int f, int32_t* xr, float* a, float* b) {
    upsample_split(x, f, xr[0], xr[1]);
    *a = (float)xr[1] / (float)(2 * f);
    upsample_spline(*a, b);
}

float hk_upsample_edge(const float* gp, const float* gq, const float* sigma) {
    return upsample_edge(gp, gq, DenoiseSigma{ sigma[0], sigma[1], sigma[2], sigma[3], sigma[4] });
}

float hk_upsample_min_weight() { return kUpsampleMinWeight; }

// ScaledTileWindow<F> of hi tile `tile` of a hi frame W wide: geom = (kFoot, kTexels, x0, y0) in lo coordinates, at[t] = the window index of the first tap of
// the wave-tiled thread t's pixel.  -> 0, or -1 for an F outside 2..4
int hk_upsample_window(int F, int tile, int W, int32_t* geom, int32_t* at) {
    if (F == 2) return window_of<2>(tile, W, geom, at);
    if (F == 3) return window_of<3>(tile, W, geom, at);
    if (F == 4) return window_of<4>(tile, W, geom, at);
    return -1;
}

}
