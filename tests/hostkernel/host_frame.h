// tests/hostkernel/host_frame.h -- TEST HARNESS ONLY, never part of the product.
//
// What the host builds of the temporal lane code share (temporal_host.cpp, moments_host.cpp): the range check every read goes through, the readers of
// whole-frame arrays by pixel index that stand in for the kernels' *Dev structs, and the camera as the bindings pass it.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../volren_amd/csrc/vr_temporal.h"

namespace {
// an index outside [0, n) is counted and not dereferenced (bad = nullptr: not checked)
struct Range {
    int64_t n;
    int64_t* bad;
    bool ok(int64_t i) const { if (!bad || (i >= 0 && i < n)) return true; ++*bad; return false; }
};
struct HostHist {
    const float* c;      // W*H*4
    const float* s;      // W*H*4: (V, N, K, D)
    Range range;
    void color(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = range.ok(i) ? c[4 * (size_t)i + k] : 0.0f; }
    void record(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = range.ok(i) ? s[4 * (size_t)i + k] : 0.0f; }
};
struct HostMoments {
    const float* m;      // W*H*4: (m1, m2, E, S)
    Range range;
    void moments(int32_t i, float o[4]) const { for (int k = 0; k < 4; ++k) o[k] = range.ok(i) ? m[4 * (size_t)i + k] : 0.0f; }
};
struct HostGuide {
    const float* g;      // W*H*8
    Range range;
    void guide(int32_t i, float o[8]) const { for (int k = 0; k < 8; ++k) o[k] = range.ok(i) ? g[8 * (size_t)i + k] : 0.0f; }
};
// a camera is 13 floats: cam_pos (3), cam_transform (9, column-major), cam_z
vr::TemporalCamera camera_of(const float* p) {
    vr::TemporalCamera c;
    std::memcpy(c.pos, p, 3 * sizeof(float));
    std::memcpy(c.m, p + 3, 9 * sizeof(float));
    c.cam_z = p[12];
    return c;
}
}  // namespace
