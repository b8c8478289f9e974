// vr_fastprobe.hip -- TEST HOOK: the VR_FAST_MATH forms of vr_math.h (neg_log_1m, sincos_, unorm8) as functions, compiled with the tolerance-mode
// flags of the vr_ptfast_* objects, so that tests can measure what each costs in accuracy (tests/test_gpu_math.py).  No render launches this.
#include <hip/hip_runtime.h>

#include "vr_device.h"
#include "vr_math.h"

#if !defined(VR_FAST_MATH)
#error "vr_fastprobe.hip is built with FASTFLAGS (-DVR_FAST_MATH=1)"
#endif

namespace vr {

__global__ void __launch_bounds__(256)
fast_math_sweep_kernel(int32_t fn, uint32_t first, float* __restrict__ out, int32_t n) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = u2f(first + (uint32_t)i);
    float r, s, c;
    switch (fn) {
    case 0: r = neg_log_1m((float)((first + (uint32_t)i) & 0xFFFFFFu) * 5.9604644775390625e-08f); break;      // the draw k 2^-24, k = first + i
    case 1: sincos_(x, s, c); r = s; break;
    case 2: sincos_(x, s, c); r = c; break;
    case 3: r = unorm8(f2u(x) & 255u); break;
    default: r = nan_(); break;
    }
    out[i] = r;
}
void launch_fast_math_sweep(int32_t fn, uint32_t first, float* out, int32_t n, hipStream_t stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(fast_math_sweep_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, first, out, n);
}

}  // namespace vr
