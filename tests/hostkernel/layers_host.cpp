// tests/hostkernel/layers_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The split and merge of the layered filter (volren_amd/csrc/vr_layers.h) compiled for the host: tests/test_layers_host.py checks them against a float64
// statement of the same definition (tests/hk_layers.py), and tests/test_gpu_layers.py checks the HIP kernels against them.
#include <stddef.h>
#include <stdint.h>

#include "../../volren_amd/csrc/vr_layers.h"

using namespace vr;

extern "C" {

// split: y, B = n*4, kappa = n -> S = n*4
void hk_layers_split(int n, const float* y, const float* B, const float* kappa, float* S) {
    for (size_t p = 0; p < (size_t)n; ++p) layers_split_pixel(y + 4 * p, B + 4 * p, kappa[p], S + 4 * p);
}

// merge: F, B = n*4, kappa = n -> out, L = n*4
void hk_layers_merge(int n, const float* F, const float* B, const float* kappa, float* out, float* L) {
    for (size_t p = 0; p < (size_t)n; ++p) layers_merge_pixel(F + 4 * p, B + 4 * p, kappa[p], L + 4 * p, out + 4 * p);
}

// the smallest filtered coverage the merge divides by
float hk_layers_min_weight() { return kLayersMinWeight; }

}
