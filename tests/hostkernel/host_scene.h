// tests/hostkernel/host_scene.h -- TEST HARNESS ONLY: the scene as the lane code sees it (SceneParams and the arrays its views point into), built on the host
// from the oracle's arrays as the product builds its device copies.  Shared by host_kernel.cpp (the lane state machine) and probe_host.cpp (the lookups).
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../volren_amd/csrc/env_pack.h"
#include "../../volren_amd/csrc/vr_trace.h"

namespace hostscene {
using namespace vr;

struct HostGrid {
    std::vector<BrickRec> recs;
    std::vector<uint8_t> atlas;
    std::vector<float> majorant, rng, atlas_f32;
    std::vector<uint16_t> majorant16;
    GridView view{};
};

inline void build_grid(HostGrid& g, const Uniforms& u, const float* lut, const uint32_t nb[3], const uint32_t* indirection, const uint32_t* range,
                const uint32_t ad[3], const uint8_t* atlas, int n_mips, const uint32_t* const* mips, bool density, bool blocked = false, bool float_atlas = true) {
    g.view.maj_blocked = blocked ? 1 : 0;
    const size_t n = (size_t)nb[0] * nb[1] * nb[2];
    const uint32_t sx = ad[0] / 8, sy = ad[1] / 8, sz = ad[2] / 8;
    for (int i = 0; i < 3; ++i) { g.view.mshift[i] = ceil_log2(nb[i]) < 3 ? 3 : ceil_log2(nb[i]); g.view.mlim[i] = (float)(8u << g.view.mshift[i]); }
    g.recs.assign(n, BrickRec{ 0u, 0.f, 0.f, 0u });
    g.atlas.assign(g.recs.size() * (size_t)kBrickBlockBytes, 0);            // brick-linear blocks == brick_grid_to_device
    for (size_t i = 0; i < n; ++i) {
        const uint32_t ind = indirection[i], rg = range[i];
        const uint32_t px = ind >> 22, py = (ind >> 12) & 1023u, pz = (ind >> 2) & 1023u;
        const float lo = half2float(rg & 0xFFFFu), hi = half2float(rg >> 16);
        const size_t idx = i;
        BrickRec& r = g.recs[idx];
        r.slot = (uint32_t)idx; r.rmin = lo; r.rdiff = hi - lo; r.range = rg;
        uint8_t* dst = &g.atlas[idx * (size_t)kBrickBlockBytes];
        if (VR_BRICK_HEADERS)
            for (uint32_t l = 0; l < 5; ++l) { memcpy(dst + l * 128u, &r.rmin, 4); memcpy(dst + l * 128u + 4u, &r.rdiff, 4); }
        if (r.rdiff != 0.f && px < sx && py < sy && pz < sz)
            for (uint32_t z = 0; z < 8; ++z) for (uint32_t y = 0; y < 8; ++y) {
                const uint8_t* src = atlas + (((size_t)(pz * 8 + z) * ad[1] + (py * 8 + y)) * ad[0] + px * 8);
                for (uint32_t x = 0; x < 8; ++x) dst[brick_voxel_byte(z * 64 + y * 8 + x)] = src[x];
            }
    }
    std::vector<uint32_t> words(range, range + n);
    uint32_t mip_off[4] = { 0u, 0u, 0u, 0u };
    for (int m = 1; m <= n_mips; ++m) {
        const uint32_t rnd = (1u << m) - 1u;
        const size_t cnt = (size_t)((nb[0] + rnd) >> m) * ((nb[1] + rnd) >> m) * ((nb[2] + rnd) >> m);
        mip_off[m] = (uint32_t)words.size();
        words.insert(words.end(), mips[m - 1], mips[m - 1] + cnt);
    }
    const uint32_t k = (uint32_t)(g.view.mshift[0] + g.view.mshift[1] + g.view.mshift[2]);
    g.majorant.assign(majorant_table_cells(k), 0.0f);
    g.majorant16.assign(majorant_table_cells(k), 0);
    g.view.maj_outside = (int32_t)majorant_padded_cells(k);
    if (density) {
        SceneParams P{}; P.u = u; P.tf_lut = lut;
        {   // == majorant_kernel: every cell without a range word (beyond the real extent, missing level, the "outside" cell) holds density_scale * 0, TF-remapped
            float m0 = u.vol_density_scale * half2float(0u);
            if (u.use_tf) { float rgba[4]; tf_lookup(P, m0 * u.vol_inv_majorant, rgba); m0 = u.vol_majorant * rgba[3]; }
            g.majorant.assign(majorant_table_cells(k), m0);
        }
        for (int mip = 0; mip <= n_mips; ++mip) {            // == majorant_kernel of vr_setup.hip
            const uint32_t rnd = (1u << mip) - 1u;
            const uint32_t dx = (nb[0] + rnd) >> mip, dy = (nb[1] + rnd) >> mip, dz = (nb[2] + rnd) >> mip;
            const uint32_t sxm = (uint32_t)g.view.mshift[0] - mip, sym = (uint32_t)g.view.mshift[1] - mip;
            for (uint32_t cz = 0; cz < dz; ++cz) for (uint32_t cy = 0; cy < dy; ++cy) for (uint32_t cx = 0; cx < dx; ++cx) {
                const uint32_t hw = words[mip_off[mip] + ((size_t)cz * dy + cy) * dx + cx] >> 16;
                const uint32_t cell = majorant_level_offset(k, mip) + majorant_cell_index(cx, cy, cz, sxm, sym, (uint32_t)mip, blocked);
                g.majorant16[cell] = (uint16_t)hw;
                float m = u.vol_density_scale * half2float(hw);
                if (u.use_tf) { float rgba[4]; tf_lookup(P, m * u.vol_inv_majorant, rgba); m = u.vol_majorant * rgba[3]; }
                g.majorant[cell] = m;
            }
        }
    }
    g.rng.resize(g.recs.size() * 2);
    for (size_t i = 0; i < g.recs.size(); ++i) { g.rng[2 * i] = g.recs[i].rmin; g.rng[2 * i + 1] = g.recs[i].rdiff; }
    g.view.bricks = g.recs.data(); g.view.atlas = g.atlas.data(); g.view.majorant = g.majorant.data();
    g.view.majorant16 = g.majorant16.data(); g.view.rng = g.rng.data();
    g.view.atlas_f32 = nullptr;
    if (density && u.use_tf && float_atlas) {                  // == RendererHIP::capture: decoded float atlas for transfer-function renders
        g.atlas_f32.resize(g.recs.size() * 512);
        for (size_t i = 0; i < g.atlas_f32.size(); ++i)
            g.atlas_f32[i] = g.rng[2 * (i >> 9)] + unorm8(g.atlas[(i >> 9) * (size_t)kBrickBlockBytes + brick_voxel_byte((uint32_t)(i & 511u))]) * g.rng[2 * (i >> 9) + 1];
        g.view.atlas_f32 = g.atlas_f32.data();
    }
    for (int i = 0; i < 3; ++i) g.view.nb[i] = (int32_t)nb[i];
    g.view.n_mips = n_mips;
}

// The paired atlas of two brick grids with the same brick layout, from vr_scene.h's description of it: per brick ten lines of 128 bytes, each
// [rmin_d, rdiff_d, rmin_e, rdiff_e | 56 x (density voxel, emission voxel)], voxels in index order (x & 7) + 8 (y & 7) + 64 (z & 7), the tenth line holding the last 8.
// Reads the grids' own blocks: five lines of [rmin, rdiff | 120 voxels].  Plain division and remainder: not the index helpers the accessors use.
inline void build_paired_atlas(const HostGrid& d, const HostGrid& e, std::vector<uint8_t>& out) {
    const size_t n = d.recs.size();
    out.assign(n * 1280u, 0);
    for (size_t b = 0; b < n; ++b) {
        const uint8_t* bd = &d.atlas[b * 640u];
        const uint8_t* be = &e.atlas[b * 640u];
        uint8_t* dst = &out[b * 1280u];
        const float head[4] = { d.recs[b].rmin, d.recs[b].rdiff, e.recs[b].rmin, e.recs[b].rdiff };
        for (uint32_t line = 0; line < 10; ++line) memcpy(dst + 128u * line, head, 16);
        for (uint32_t v = 0; v < 512; ++v) {
            const uint32_t src = 128u * (v / 120u) + 8u + v % 120u;
            const uint32_t at = 128u * (v / 56u) + 16u + 2u * (v % 56u);
            dst[at] = bd[src];
            dst[at + 1u] = be[src];
        }
    }
}

struct hk_grid_desc {
    uint32_t nb[3]; uint32_t atlas_dim[3]; int32_t n_mips;
    const uint32_t* indirection; const uint32_t* range; const uint8_t* atlas; const uint32_t* mips[3];
    const uint16_t* dense; uint32_t dim[3];
};

// the scene as the lane code sees it (SceneParams + the arrays its views point into), built from the oracle's arrays exactly as the product builds its device copies
struct HostScene {
    SceneParams P{};
    HostGrid dg, eg;
    std::vector<uint16_t> blocked;
    std::vector<float> env, cdf;
    std::vector<uint32_t> rgbe;
    std::vector<uint8_t> paired;          // the paired atlas (build_paired_atlas); the views of P do not point into it
};
// flags of build_scene
// (8 belongs to probe_host.cpp: pair the atlases.)  HS_MAJ_LINEAR: a linear majorant table whatever HS_MAJ_BLOCKED and VR_HOST_MAJ_BLOCKED say
enum { HS_MAJ_BLOCKED = 1, HS_NO_FLOAT_ATLAS = 2, HS_NO_COMPACT_ENV = 4, HS_MAJ_LINEAR = 16 };
inline void build_scene(HostScene& S, const Uniforms* up, const hk_grid_desc* density, const hk_grid_desc* emission, const float* lut,
                        const float* env_rgb, int env_w, int env_h, const float* impmap, int imp_dim, int flags = 0) {
    SceneParams& P = S.P;
    HostGrid& dg = S.dg; HostGrid& eg = S.eg;
    std::vector<uint16_t>& blocked = S.blocked;
    std::vector<float>& env = S.env; std::vector<float>& cdf = S.cdf;
    const Uniforms& u = *up;
    P.u = u;
    build_grid(dg, u, lut, density->nb, density->indirection, density->range, density->atlas_dim, density->atlas, density->n_mips, density->mips, true,
               // the majorant table's levels 0-1 in 4x4x4-cell blocks (a per-grid choice of the product since round 5; the lane code reads the view's flag at run time here)
               (flags & HS_MAJ_LINEAR) == 0 && ((flags & HS_MAJ_BLOCKED) != 0 || (std::getenv("VR_HOST_MAJ_BLOCKED") != nullptr && std::getenv("VR_HOST_MAJ_BLOCKED")[0] == '1')),
               (flags & HS_NO_FLOAT_ATLAS) == 0);
    P.density = dg.view;
    // (blocked: == dense_grid_to_device: 4x4x4 blocks)
    if (density->dense) {
        const uint32_t dx = density->dim[0], dy = density->dim[1], dz = density->dim[2];
        const uint32_t bx = (dx + 3u) / 4u, by = (dy + 3u) / 4u, bz = (dz + 3u) / 4u;
        blocked.assign((size_t)bx * by * bz * 64u, 0);
        for (uint32_t z = 0; z < dz; ++z) for (uint32_t y = 0; y < dy; ++y) for (uint32_t x = 0; x < dx; ++x)
            blocked[dense_blocked_index(x, y, z, bx, by)] = density->dense[((size_t)z * dy + y) * dx + x];
        P.density.dense = blocked.data();
        P.density.dblk[0] = (int32_t)bx; P.density.dblk[1] = (int32_t)by;
    }
    for (int i = 0; i < 3; ++i) P.density.dim[i] = (int32_t)density->dim[i];
    if (emission && u.has_emission) {
        build_grid(eg, u, lut, emission->nb, emission->indirection, emission->range, emission->atlas_dim, emission->atlas, emission->n_mips, emission->mips, false);
        P.emission = eg.view;
        // emission_from_density = vol_emission_inv_transform * vol_density_transform (same product as hostmath.h)
        const float* a = u.vol_emission_inv_transform; const float* b = u.vol_density_transform;
        for (int c = 0; c < 4; ++c) for (int r = 0; r < 4; ++r)
            P.emission_from_density[4 * c + r] = a[r] * b[4 * c] + a[4 + r] * b[4 * c + 1] + a[8 + r] * b[4 * c + 2] + a[12 + r] * b[4 * c + 3];
    }
    P.tf_lut = lut;
    env.assign((size_t)env_w * env_h * kEnvTexelFloats, 0.0f);
    for (size_t i = 0; i < (size_t)env_w * env_h; ++i) for (int k = 0; k < 3; ++k) env[kEnvTexelFloats * i + k] = env_rgb[3 * i + k];
    P.envmap = env.data(); P.env_w = env_w; P.env_h = env_h;
    // == Environment::build: the compact map when every texel has that form, and the pyramid's coarsest value as an argument
    P.env_rgbe = (!(flags & HS_NO_COMPACT_ENV) && pack_rgbe_map(env.data(), (size_t)env_w * env_h, kEnvTexelFloats, S.rgbe)) ? S.rgbe.data() : nullptr;
    P.impmap = impmap; P.imp_dim = imp_dim;
    int base = 0; while ((1 << base) < imp_dim) ++base;
    P.env_avg_w = impmap[imp_level_offset(imp_dim, base)]; P.env_avg_w_set = 1;
    bool div_safe = true;
    cdf.assign(env_cdf_table_floats(base - 1), 0.0f);
    {   // == env_cdf_kernel of vr_setup.hip
        for (int mip = base - 1; mip >= 0; --mip) {
            const int d = imp_dim >> mip, hd = d >> 1;
            const float* level = impmap + imp_level_offset(imp_dim, mip);
            for (int y = 0; y < hd; ++y) for (int x = 0; x < hd; ++x) {
                const float w0 = level[(size_t)(2 * y) * d + 2 * x], w1 = level[(size_t)(2 * y) * d + 2 * x + 1];
                const float w2 = level[(size_t)(2 * y + 1) * d + 2 * x], w3 = level[(size_t)(2 * y + 1) * d + 2 * x + 1];
                const float q0 = w0 + w2, q1 = w1 + w3;
                float* o = cdf.data() + env_cdf_index(base - 1, base - 1 - mip, (uint32_t)x, (uint32_t)y);
                o[0] = q0 / max_(1e-8f, q0 + q1); o[1] = w0 / q0; o[2] = w1 / q1;
                for (int j = 0; j < 3; ++j) { const float v = o[j]; div_safe = div_safe && (v != v || v == 0.0f || (v >= 1.3234890e-23f && v <= 1.0f)); }
                if (mip == 0) { o[3] = w0; o[4] = w1; o[5] = w2; o[6] = w3; }
            }
        }
    }
    P.env_cdf = cdf.data();
    P.env_div_safe = div_safe ? 1 : 0;
    P.cam_z = -0.5f / tan_(0.5f * kPi * u.cam_fov / 180.f);
}

}  // namespace hostscene
