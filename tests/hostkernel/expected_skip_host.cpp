// tests/hostkernel/expected_skip_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// The clear-distance table (volren_amd/csrc/vr_clear.h) and the expected-value march that skips by it (vr_expected.h, SKIP) compiled for the host, on the
// scene host_scene.h builds from the oracle's arrays: tests/test_expected_skip_host.py checks the table against a numpy statement of its definition and the
// march with the table against the march without, bit for bit; tests/test_gpu_expected_skip.py checks the HIP kernels against both.
#include "host_scene.h"

#include "../../volren_amd/csrc/vr_expected.h"

using namespace hostscene;

namespace {

// == launch_clear_table of vr_setup.hip: the marking pass, then one pass per axis, each from one buffer into the other
void build_table(const GridView& g, std::vector<uint8_t>& table, int32_t n[3]) {
    clear_cells(g, n);
    const size_t cells = (size_t)n[0] * n[1] * n[2];
    std::vector<uint8_t> scratch(cells);
    table.assign(cells, 0);
    for (int32_t cz = 0; cz < n[2]; ++cz) for (int32_t cy = 0; cy < n[1]; ++cy) for (int32_t cx = 0; cx < n[0]; ++cx)
        scratch[((size_t)cz * n[1] + cy) * n[0] + cx] = clear_box_bits(g, cx, cy, cz, 0, 1) != 0u ? (uint8_t)0 : (uint8_t)kClearMax;
    uint8_t* buf[2] = { scratch.data(), table.data() };
    for (int axis = 0; axis < 3; ++axis) {
        const uint8_t* in = buf[axis & 1];
        uint8_t* out = buf[(axis + 1) & 1];
        for (int32_t cz = 0; cz < n[2]; ++cz) for (int32_t cy = 0; cy < n[1]; ++cy) for (int32_t cx = 0; cx < n[0]; ++cx)
            out[((size_t)cz * n[1] + cy) * n[0] + cx] = (uint8_t)clear_axis_pass(in, n, axis, cx, cy, cz);
    }
}

template <bool TF, bool SKIP, bool AUDIT>
void pixel(const SceneParams& P, int x, int y, int rays, float* o, ExpectedRayInfo* ri, const ClearTable* C, ExpectedWork* w) {
    expected_pixel<TF, true, SKIP, true, AUDIT>(P, x, y, rays, o, ri, C, w);
}

}  // namespace

extern "C" {

// the extent of the density grid's table in cells; out (may be null): the table, x fastest
void hk_clear_table(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                    const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, uint8_t* out, int32_t* cells) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    std::vector<uint8_t> table;
    int32_t n[3];
    build_table(S.P.density, table, n);
    for (int i = 0; i < 3; ++i) cells[i] = n[i];
    if (out) memcpy(out, table.data(), table.size());
}

// hk_expected_pass of expected_host.cpp with the table: skip 0 marches every step, 1 skips by the table, 2 skips and audits (every dropped step is evaluated in
// full all the same).  work: 5 sums over the frame -- sub-rays marched, steps reached, steps that fetched, table reads, dropped steps with sigma > 0 (audit only)
void hk_expected_skip_pass(const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                           const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int rays, int skip, float* out, int32_t* info,
                           uint64_t* work) {
    HostScene S;
    build_scene(S, up, density, emission, lut, env_rgb, env_w, env_h, impmap, imp_dim);
    const SceneParams& P = S.P;
    std::vector<uint8_t> table;
    ClearTable C = { nullptr, { 0, 0, 0 } };
    if (skip) { build_table(P.density, table, C.n); C.d = table.data(); }
    const int W = P.u.resolution[0], H = P.u.resolution[1];
    const bool tf = P.u.use_tf != 0;
    ExpectedRayInfo ri[16];
    for (int k = 0; k < 5; ++k) work[k] = 0;
    for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) {
        const size_t p = (size_t)y * W + x;
        float* o = out + 8 * p;
        ExpectedWork w = { 0u, 0u, 0u, 0u, 0u };
        if (skip == 0) { if (tf) pixel<true, false, false>(P, x, y, rays, o, ri, nullptr, &w); else pixel<false, false, false>(P, x, y, rays, o, ri, nullptr, &w); }
        else if (skip == 1) { if (tf) pixel<true, true, false>(P, x, y, rays, o, ri, &C, &w); else pixel<false, true, false>(P, x, y, rays, o, ri, &C, &w); }
        else { if (tf) pixel<true, true, true>(P, x, y, rays, o, ri, &C, &w); else pixel<false, true, true>(P, x, y, rays, o, ri, &C, &w); }
        work[0] += w.rays; work[1] += w.steps; work[2] += w.fetched; work[3] += w.reads; work[4] += w.audit;
        if (info)
            for (int k = 0; k < rays * rays; ++k) {
                int32_t* d = info + 3 * (p * (size_t)(rays * rays) + (size_t)k);
                d[0] = ri[k].m; d[1] = ri[k].steps; d[2] = (int32_t)f2u(ri[k].T);
            }
    }
}

}
