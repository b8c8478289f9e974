// vr_probe.hip -- test hooks: the device side of vr_probe.h (scene-data lookups) and of vr_math_probe.h (the math layer).  One thread per item;
// nothing a render launches.
#include <hip/hip_runtime.h>

#include "vr_device.h"
#include "vr_math_probe.h"
#include "vr_probe.h"

namespace vr {

__global__ void __launch_bounds__(256)
probe_kernel(const SceneParams P, int32_t what, int32_t form, const uint32_t* __restrict__ in, float* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float o[7] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    const uint4 w4 = reinterpret_cast<const uint4*>(in)[i];
    const uint32_t w[4] = { w4.x, w4.y, w4.z, w4.w };
    probe_item(P, what, form, w, o);
    const int32_t k = probe_out_words(what);
    for (int32_t j = 0; j < k; ++j) out[(size_t)i * (uint32_t)k + (uint32_t)j] = o[j];
}

void launch_probe(const SceneParams& P, int32_t what, int32_t form, const uint32_t* in, float* out, uint32_t n, hipStream_t stream) {
    if (n == 0u) return;
    hipLaunchKernelGGL(probe_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, P, what, form, in, out, n);
}

__global__ void __launch_bounds__(256)
math_probe_kernel(int32_t fn, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int32_t n) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = a[i], y = b[i];
    float r;
    if (fn == 17) { const v3 q = rcp3_exact(v3{ x, y, x }); r = q.y; }      // the three-at-once form: y's reciprocal, range test shared with x
    else r = math_probe_eval(fn, x, y);
    out[i] = r;
}
// the same over a range of bit patterns: x = bits(first + i) (wrapping), y one value; only the results leave the device
__global__ void __launch_bounds__(256)
math_sweep_kernel(int32_t fn, uint32_t first, float y, float* __restrict__ out, int32_t n) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = math_probe_eval(fn, u2f(first + (uint32_t)i), y);
}
void launch_math_probe(int32_t fn, const float* a, const float* b, float* out, int32_t n, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(math_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, a, b, out, n);
}
void launch_math_sweep(int32_t fn, uint32_t first, float b, float* out, int32_t n, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(math_sweep_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, first, b, out, n);
}

}  // namespace vr
