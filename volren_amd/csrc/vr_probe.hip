// vr_probe.hip -- test hooks: the device side of vr_probe.h (scene-data lookups), of vr_path_probe.h (the per-path layer) and of vr_math_probe.h (the math layer).  One thread per item;
// nothing a render launches.
#include <hip/hip_runtime.h>

#include "vr_device.h"
#include "vr_math_probe.h"
#include "vr_path_probe.h"
#include "vr_pathtrace.h"
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

// the per-path layer (vr_path_probe.h): the scene-free kinds in one kernel, a segment kernel per compiled instance
__global__ void __launch_bounds__(256)
path_probe_kernel(const SceneParams P, int32_t kind, int32_t form, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t ki = (uint32_t)path_probe_in_words(kind), ko = (uint32_t)path_probe_out_words(kind);
    uint32_t w[9] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u }, o[5] = { 0u, 0u, 0u, 0u, 0u };
    for (uint32_t j = 0; j < ki; ++j) w[j] = in[(size_t)i * ki + j];
    path_probe_item(P, kind, form, w, o);
    for (uint32_t j = 0; j < ko; ++j) out[(size_t)i * ko + j] = o[j];
}
// the probe's statement of the early collision tail (vr_path_probe.h, also compiled for the host, where vr_pathtrace.h is not) against the scheduler's own rule:
// every build of the library checks that the probe runs collide_finish in the form the kernel of that instance calls
template <int FORM, bool TF> constexpr bool path_early_agrees() {
    using K = typename PathInstance<FORM, TF>::K;
    return path_collide_early<K>() == collide_tail_early<K, false>();
}
template <int FORM> constexpr bool path_early_agrees_from() { return path_early_agrees<FORM, false>() && path_early_agrees<FORM, true>() && path_early_agrees_from<FORM + 1>(); }
template <> constexpr bool path_early_agrees_from<kPtInstances>() { return true; }
static_assert(path_early_agrees_from<0>(), "vr_path_probe.h path_collide_early differs from vr_pathtrace.h collide_tail_early");

template <int FORM>
__global__ void __launch_bounds__(256)
path_segment_kernel(const SceneParams P, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t w[8], o[14];
    for (uint32_t j = 0; j < 8u; ++j) w[j] = in[(size_t)i * 8u + j];
    path_segment_form<FORM>(P, w, o);
    for (uint32_t j = 0; j < 14u; ++j) out[(size_t)i * 14u + j] = o[j];
}
void launch_path_probe(const SceneParams& P, int32_t kind, int32_t form, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream) {
    if (n == 0u) return;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (kind != PATH_SEGMENT) { hipLaunchKernelGGL(path_probe_kernel, grid, block, 0, stream, P, kind, form, in, out, n); return; }
    switch (form) {
    case 0: hipLaunchKernelGGL(path_segment_kernel<0>, grid, block, 0, stream, P, in, out, n); break;
    case 1: hipLaunchKernelGGL(path_segment_kernel<1>, grid, block, 0, stream, P, in, out, n); break;
    case 2: hipLaunchKernelGGL(path_segment_kernel<2>, grid, block, 0, stream, P, in, out, n); break;
    case 3: hipLaunchKernelGGL(path_segment_kernel<3>, grid, block, 0, stream, P, in, out, n); break;
    case 4: hipLaunchKernelGGL(path_segment_kernel<4>, grid, block, 0, stream, P, in, out, n); break;
    case 5: hipLaunchKernelGGL(path_segment_kernel<5>, grid, block, 0, stream, P, in, out, n); break;
    case 6: hipLaunchKernelGGL(path_segment_kernel<6>, grid, block, 0, stream, P, in, out, n); break;
    default: break;
    }
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
