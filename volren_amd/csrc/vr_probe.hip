// vr_probe.hip -- test hook: the device side of vr_probe.h.  One thread per item; nothing a render launches.
#include <hip/hip_runtime.h>

#include "vr_device.h"
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

}  // namespace vr
