// tests/hostkernel/hotpair_host.cpp -- TEST HARNESS ONLY, never part of the product.
//
// Two pieces of the hot pair (volren_amd/csrc/vr_trace.h) compiled for the host, for tests/test_collide_shadow_host.py and tests/test_gather_addressing_host.py.
//
// (1) collide_finish of volren_amd/csrc/vr_trace.h -- the function the HIP kernels run at a tentative collision -- compiled for the host and called on crafted
// states of a SHADOW segment of the DDA trackers: tests/test_collide_shadow_host.py holds what it leaves (Tr, state, the RNG state, tau) against
// transmittanceDDA's expression written out there, bit for bit -- also where a cell's majorant exceeds the volume's, is zero, negative or NaN, which no
// scene the product builds produces and which is the only way past the shortcut for blocked shadow rays (VR_SHADOW_BLOCKED_SHORTCUT).
// -DVR_SHADOW_BLOCKED_SHORTCUT=0 builds the function without the shortcut (the test runs both).
//
// (2) The gathers' two addressing forms (table_load / line_load: 32-bit byte offsets from the table's base, or 64-bit addresses) on the same tables, element by element,
// and the rule that chooses between them per launch (vr_scene.h grid_largest_table_bytes) on extents the test names -- no GPU test can afford a 4 GiB grid.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../volren_amd/csrc/vr_trace.h"

using namespace vr;

namespace {
struct ColdHost {
    float v[C_COUNT];
    float ld(int32_t f) const { return v[f]; }
    void st(int32_t f, float x) { v[f] = x; }
};
template <class K>
void run(const uint32_t* in, uint32_t* out) {
    SceneParams P{};
    P.u.vol_majorant = u2f(in[2]);
    P.u.vol_inv_majorant = 1.0f / P.u.vol_majorant;
    P.u.vol_density_scale = 1.0f;
    Hot h{};
    h.seed = in[0];
    h.majorant = u2f(in[1]);
    h.Tr = u2f(in[3]);
    h.shadow = 1;
    h.state = ST_COLLIDE;
    h.mipq = 12;
    h.far = 1.0f;
    CollideIO<K> io{};
    io.a.in = true;                     // the tap's value: rmin + unorm8(0) * 0 = the density given
    io.d.rmin = u2f(in[4]);
    ColdHost c{};
    collide_finish<K>(h, c, P, io, nullptr);
    out[0] = f2u(h.Tr); out[1] = (uint32_t)h.state; out[2] = h.seed; out[3] = f2u(h.tau); out[4] = (uint32_t)h.mipq;
}
}  // namespace

extern "C" {

int hc_shortcut_compiled() { return VR_SHADOW_BLOCKED_SHORTCUT ? 1 : 0; }

// in: [n][5] = RNG state, cell majorant, vol_majorant, Tr, density at the collision point (floats as bit patterns)
// out: [n][5] = Tr, state, RNG state, tau, mipq after collide_finish
// form 0: the kernel of one scene kind (DDA trackers, brick grid, no transfer function: the quotient by div_core); 1: everything decided at run time (the IEEE quotient)
int hc_shadow_collide(int form, long long n, const uint32_t* in, uint32_t* out) {
    if (form != 0 && form != 1) return 1;
    for (long long i = 0; i < n; ++i) {
        if (form == 0) run<TraceCfg<false, 0, 0, 0, 2>>(in + 5 * i, out + 5 * i);
        else run<TraceCfg<false, 2, 2, 2, 2>>(in + 5 * i, out + 5 * i);
    }
    return 0;
}

// grid_largest_table_bytes of a view with these extents: brick grid nb[3] (dense == 0) or dense grid dim[3]; mshift[3] as commit() sets them
unsigned long long hc_largest_table_bytes(const int32_t nb[3], const int32_t mshift[3], const int32_t dim[3], int dense, int float_atlas, int paired, int tf) {
    static const uint16_t some_voxels[1] = { 0 };
    static const float some_floats[1] = { 0.0f };
    GridView g{};
    for (int i = 0; i < 3; ++i) { g.nb[i] = nb[i]; g.mshift[i] = mshift[i]; g.dim[i] = dim[i]; }
    g.dblk[0] = (dim[0] + 3) / 4; g.dblk[1] = (dim[1] + 3) / 4;
    if (dense) g.dense = some_voxels;
    if (float_atlas) g.atlas_f32 = some_floats;
    return grid_largest_table_bytes(g, paired != 0, tf != 0);
}

// Every element of small tables through both forms: a brick atlas of `records` blocks (all 512 voxels of each, range and byte), its decoded float atlas (the 8 corners
// of trilinear_load), a dense grid of `records` 4x4x4 blocks, and fp16 / float majorant tables of `cells` cells.  Returns the number of elements that differ (0), or -1
// when the tables' contents were not all distinct enough to tell neighbours apart.
long long hc_addressing_forms_differ(int records, int cells) {
    std::vector<uint8_t> atlas((size_t)records * kBrickBlockBytes);
    uint32_t s = 12345u;
    for (auto& b : atlas) { s = s * 1664525u + 1013904223u; b = (uint8_t)(s >> 24); }
    std::vector<float> f32((size_t)records * 512u);
    for (size_t i = 0; i < f32.size(); ++i) f32[i] = (float)i + 0.5f;
    std::vector<uint16_t> dense((size_t)records * 64u), maj16((size_t)cells);
    for (size_t i = 0; i < dense.size(); ++i) dense[i] = (uint16_t)(i * 40503u >> 3);
    for (size_t i = 0; i < maj16.size(); ++i) maj16[i] = (uint16_t)(i * 25171u >> 2);
    std::vector<float> maj((size_t)cells);
    for (size_t i = 0; i < maj.size(); ++i) maj[i] = 1.0f + (float)i;
    GridView gb{}, gd{}, gf{};
    gb.atlas = atlas.data(); gb.majorant16 = maj16.data(); gb.majorant = maj.data();
    gd.dense = dense.data();
    gf.atlas = atlas.data(); gf.atlas_f32 = f32.data();
    long long bad = 0;
    for (uint32_t c = 0; c < (uint32_t)records; ++c)
        for (uint32_t o = 0; o < 512u; ++o) {
            const TapAddr a{ c, o, true };
            const TapData x = tap_load<0, 0, true>(gb, a), y = tap_load<0, 0, false>(gb, a);
            bad += (f2u(x.rmin) != f2u(y.rmin)) + (f2u(x.rdiff) != f2u(y.rdiff)) + (x.raw != y.raw);
            if (o < 64u) { const TapAddr b{ c, o, true }; bad += tap_load<1, 0, true>(gd, b).raw != tap_load<1, 0, false>(gd, b).raw; }
        }
    for (uint32_t c = 0; c + 8u <= (uint32_t)records * 64u; c += 5u) {          // eight corners at a time, as the transfer-function kernels load them
        TriIO x{}, y{};
        for (uint32_t n = 0; n < 8u; ++n) { x.a[n] = y.a[n] = TapAddr{ (c + n) >> 6, ((c + n) & 63u) * 8u + n, true }; }
        trilinear_load<0, 0, true>(gf, x); trilinear_load<0, 0, false>(gf, y);
        for (uint32_t n = 0; n < 8u; ++n) bad += x.d[n].raw != y.d[n].raw;
    }
    for (int32_t i = 0; i < cells; ++i) {
        bad += majorant_fetch<false, true>(gb, i) != majorant_fetch<false, false>(gb, i);
        bad += majorant_fetch<true, true>(gb, i) != majorant_fetch<true, false>(gb, i);
    }
    return bad;
}

}  // extern "C"
