// tests/hostkernel/expected_cubic_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The cubic B-spline lookup (volren_amd/csrc/vr_cubic.h), the clear-distance table of either reach (vr_clear.h) and the expected-value march on either
// field (vr_expected.h, CUBIC) compiled for the host, on the scene host_scene.h builds from the oracle's arrays: tests/test_expected_cubic_host.py checks
// them against float64 and numpy statements of their definitions (tests/hk_expected_cubic.py); tests/test_gpu_expected_cubic.py checks the HIP kernels
// against them.  Built with -DVR_HOST_TRACE: the sink below holds every tap the lookups make to the extent of the table it names and counts what falls
// outside (hc_violations); the tests assert 0.
#include <atomic>

#include "host_scene.h"

#include "../../volren_amd/csrc/vr_expected.h"

using namespace hostscene;

namespace {
const HostScene* g_scene = nullptr;      // the scene of the running call (one at a time)
std::atomic<long long> g_violations{ 0 }, g_taps{ 0 };
}  // namespace

namespace vr {
void host_trace(int32_t cls, const void* table, size_t a, size_t b) {
    const HostScene* S = g_scene;
    if (!S || cls != TR_TAP) return;
    g_taps.fetch_add(1, std::memory_order_relaxed);
    bool ok = false;
    // a: brick record (or 4x4x4 block of a dense grid), b: voxel inside it; a dense grid's view may also carry the brick atlas of its descriptor and name itself by it
    if (!S->blocked.empty() && (table == (const void*)S->blocked.data() || table == (const void*)S->dg.atlas.data())) ok = b < 64u && a * 64u + b < S->blocked.size();
    else if (table == (const void*)S->dg.atlas.data()) ok = b < 512u && a < S->dg.recs.size();
    if (!ok) g_violations.fetch_add(1, std::memory_order_relaxed);
}
}  // namespace vr

namespace {

// == launch_clear_table of vr_setup.hip at that reach
void build_table(const GridView& g, int reach, std::vector<uint8_t>& table, int32_t n[3]) {
    clear_cells(g, n);
    const size_t cells = (size_t)n[0] * n[1] * n[2];
    std::vector<uint8_t> scratch(cells);
    table.assign(cells, 0);
    for (int32_t cz = 0; cz < n[2]; ++cz) for (int32_t cy = 0; cy < n[1]; ++cy) for (int32_t cx = 0; cx < n[0]; ++cx)
        scratch[((size_t)cz * n[1] + cy) * n[0] + cx] = clear_box_bits(g, cx, cy, cz, 0, 1, reach) != 0u ? (uint8_t)0 : (uint8_t)kClearMax;
    uint8_t* buf[2] = { scratch.data(), table.data() };
    for (int axis = 0; axis < 3; ++axis) {
        const uint8_t* in = buf[axis & 1];
        uint8_t* out = buf[(axis + 1) & 1];
        for (int32_t cz = 0; cz < n[2]; ++cz) for (int32_t cy = 0; cy < n[1]; ++cy) for (int32_t cx = 0; cx < n[0]; ++cx)
            out[((size_t)cz * n[1] + cy) * n[0] + cx] = (uint8_t)clear_axis_pass(in, n, axis, cx, cy, cz);
    }
}

template <bool TF, bool SKIP, bool AUDIT, bool CUBIC>
void pixel(const SceneParams& P, int x, int y, int rays, float* o, ExpectedRayInfo* ri, const ClearTable* C, ExpectedWork* w) {
    expected_pixel<TF, true, SKIP, true, AUDIT, CUBIC>(P, x, y, rays, o, ri, C, w);
}
template <bool TF, bool CUBIC>
void pixel_of(int skip, const SceneParams& P, int x, int y, int rays, float* o, ExpectedRayInfo* ri, const ClearTable* C, ExpectedWork* w) {
    if (skip == 0) pixel<TF, false, false, CUBIC>(P, x, y, rays, o, ri, nullptr, w);
    else if (skip == 1) pixel<TF, true, false, CUBIC>(P, x, y, rays, o, ri, C, w);
    else pixel<TF, true, true, CUBIC>(P, x, y, rays, o, ri, C, w);
}

}  // namespace

extern "C" {

// taps that fell outside their table since the last reset, and the taps checked
long long hc_violations() { return g_violations.load(); }
long long hc_taps() { return g_taps.load(); }
void hc_reset() { g_violations = 0; g_taps = 0; }

// cubic_lookup on the density grid at n index-space points (3 floats each, passed as their bits): out = n x (value, gx, gy, gz)
void hc_cubic_probe(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                    const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, const uint32_t* pts, long long n, float* out) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    g_scene = &S;
    for (long long i = 0; i < n; ++i) {
        v3 g{ 0.0f, 0.0f, 0.0f };
        cubic_lookup(S.P.density, v3{ u2f(pts[3 * i]), u2f(pts[3 * i + 1]), u2f(pts[3 * i + 2]) }, out[4 * i], g);
        out[4 * i + 1] = g.x; out[4 * i + 2] = g.y; out[4 * i + 3] = g.z;
    }
    g_scene = nullptr;
}

// the density grid's table of reach 1 or 2; out (may be null): the table, x fastest
void hc_clear_table(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                    const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int reach, uint8_t* out, int32_t* cells) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    std::vector<uint8_t> table;
    int32_t n[3];
    build_table(S.P.density, reach, table, n);
    for (int i = 0; i < 3; ++i) cells[i] = n[i];
    if (out) memcpy(out, table.data(), table.size());
}

// hk_expected_skip_pass of expected_skip_host.cpp with the field: field 0 marches the trilinear field, 1 the tracker's (CUBIC; under a LUT the trilinear one).
// skip 0 marches every step, 1 skips by the table, 2 skips and audits.  reach: the table's, 0 = the one the field marches with (1 or 2) -- anything else is a
// test of the test: CUBIC with the table of reach 1 drops steps that count.  work: rays, steps, fetched, reads, audit.
void hc_expected_pass(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                      const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int rays, int field, int skip, int reach, float* out,
                      int32_t* info, uint64_t* work) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    const bool tf = P.u.use_tf != 0, cubic = field != 0 && !tf;
    std::vector<uint8_t> table;
    ClearTable C = { nullptr, { 0, 0, 0 } };
    if (skip) { build_table(P.density, reach ? reach : (cubic ? 2 : 1), table, C.n); C.d = table.data(); }
    const int W = P.u.resolution[0], H = P.u.resolution[1];
    ExpectedRayInfo ri[16];
    for (int k = 0; k < 5; ++k) work[k] = 0;
    g_scene = &S;
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        float* o = out + 8 * p;
        ExpectedWork w = { 0u, 0u, 0u, 0u, 0u };
        if (tf) { if (field) pixel_of<true, true>(skip, P, x, y, rays, o, ri, &C, &w); else pixel_of<true, false>(skip, P, x, y, rays, o, ri, &C, &w); }
        else if (cubic) pixel_of<false, true>(skip, P, x, y, rays, o, ri, &C, &w);
        else pixel_of<false, false>(skip, P, x, y, rays, o, ri, &C, &w);
        work[0] += w.rays; work[1] += w.steps; work[2] += w.fetched; work[3] += w.reads; work[4] += w.audit;
        if (info)
            for (int k = 0; k < rays * rays; ++k) {
                int32_t* d = info + 3 * (p * (size_t)(rays * rays) + (size_t)k);
                d[0] = ri[k].m; d[1] = ri[k].steps; d[2] = (int32_t)f2u(ri[k].T);
            }
    }
    g_scene = nullptr;
}

}
