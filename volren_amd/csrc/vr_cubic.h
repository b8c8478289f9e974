// vr_cubic.h -- the mean field of the stochastic-tricubic tap: the separable cubic B-spline of the voxels, value and gradient from one set of 64 taps.
//
// Without a LUT the tracker decides every tentative collision on ONE tap of the 4x4x4 neighbourhood, drawn with the B-spline weights (vr_trace.h
// tricubic_tap, common.glsl:221-244): an unbiased estimate of the weighted sum below, so delta tracking runs on that sum.  The expected-value march
// (vr_expected.h, CUBIC) integrates it instead of the trilinear field.  The reservoir's max(1e-3, .) guards are not restated: the partial sums of
// the weights are at least 1/6 from the second tap on, so the selection probabilities are the weights to float rounding.
//
// The lookup, operation by operation in float32 (this text is the specification; tests/hk_expected_cubic.py restates it in float64).  No operation is
// contracted but where fma_ is written.
//   Axis      q = ip - 0.5f, fl = floor_(q), t = q - fl, t2 = t * t, k = 1.0f / 6.0f.  Weights, as tricubic_axis_weights writes them, left to right:
//               w0 = k * (-t * t2 + 3.0f * t2 - 3.0f * t + 1.0f)      w1 = k * (3.0f * t * t2 - 6.0f * t2 + 4.0f)
//               w2 = k * (-3.0f * t * t2 + 3.0f * t2 + 3.0f * t + 1.0f)   w3 = k * t * t2
//             and their derivatives by t:
//               d0 = 0.5f * (-t2 + 2.0f * t - 1.0f)   d1 = 0.5f * (3.0f * t2 - 4.0f * t)   d2 = 0.5f * (-3.0f * t2 + 2.0f * t + 1.0f)   d3 = 0.5f * t2
//   Taps      voxels fl - 1 .. fl + 2 per axis, v[k][j][i] (z, y, x), decoded as tap_value decodes them from the byte atlas or the fp16 voxels; +0 outside
//             the grid.  An axis is in range when fl >= -2 and fl <= extent, compared as floats (NaN fails) BEFORE anything is converted: only then is fl
//             converted, exactly; otherwise the axis has no tap inside, and neither has the lookup.  No address is formed from a coordinate that is not
//             finite or lies far outside; the weights are what the lines above make of it (NaN for an infinite or NaN coordinate, and then so is the result).
//   Sums      dot4(a, x) = fma_(a3, x3, fma_(a2, x2, fma_(a1, x1, a0 * x0))).  Per row r[k][j] = dot4(wx, v[k][j]), rx[k][j] = dot4(dx, v[k][j]); per
//             slab s[k] = dot4(wy, r[k]), sx[k] = dot4(wy, rx[k]), sy[k] = dot4(dy, r[k]); then raw = dot4(wz, s) and the gradient in voxel units
//             (dot4(wz, sx), dot4(wz, sy), dot4(dz, s)): the same 64 values with one axis' weights replaced by its derivatives.  No further loads.
// The 64 taps lie in at most 2 x 2 x 2 cells (bricks of 8^3 voxels, 4^3 blocks of a dense grid): per axis the taps inside the grid are a run whose first
// and last cell are the only two it touches.  The eight cells' indices -- and a brick's decode range, which every line of its block repeats -- are formed
// once per lookup; a tap selects among them and adds its voxel's place.  A tap outside the grid reads a voxel of a cell inside (unconditional loads) and
// is discarded.
#pragma once

#include "vr_trace.h"

namespace vr {

struct CubicAxis {
    float w[4], d[4];
    uint32_t lo, hi;          // cells of the first and the last tap inside the grid (0, 0 without one)
    uint32_t off[4];          // a tap's place inside its cell along this axis (0 outside the grid)
    bool in[4], up[4];        // inside the grid; in cell hi and hi != lo
};

VR_HD float cubic_dot4(const float a[4], float x0, float x1, float x2, float x3) { return fma_(a[3], x3, fma_(a[2], x2, fma_(a[1], x1, a[0] * x0))); }

// one axis of the lookup at coordinate c of a grid of `extent` voxels in cells of 2^lg
VR_HD void cubic_axis(float c, uint32_t extent, uint32_t lg, CubicAxis& a) {
    const float q = c - 0.5f;
    const float fl = floor_(q);
    const float t = q - fl, t2 = t * t;
    const float k = 1.0f / 6.0f;
    a.w[0] = k * (-t * t2 + 3.0f * t2 - 3.0f * t + 1.0f);
    a.w[1] = k * (3.0f * t * t2 - 6.0f * t2 + 4.0f);
    a.w[2] = k * (-3.0f * t * t2 + 3.0f * t2 + 3.0f * t + 1.0f);
    a.w[3] = k * t * t2;
    a.d[0] = 0.5f * (-t2 + 2.0f * t - 1.0f);
    a.d[1] = 0.5f * (3.0f * t2 - 4.0f * t);
    a.d[2] = 0.5f * (-3.0f * t2 + 2.0f * t + 1.0f);
    a.d[3] = 0.5f * t2;
    // in range on the floats (extent < 2^24: exact), after which the conversion is exact; an axis out of range starts at -4: all four taps negative
    const bool ok = (fl >= -2.0f) & (fl <= (float)extent);
    const int32_t i0 = ok ? (int32_t)fl - 1 : -4;
    const int32_t first = i0 > 0 ? i0 : 0, last = i0 + 3 < (int32_t)extent - 1 ? i0 + 3 : (int32_t)extent - 1;
    const bool any = first <= last;
    a.lo = any ? (uint32_t)first >> lg : 0u;
    a.hi = any ? (uint32_t)last >> lg : 0u;
    const uint32_t mask = (1u << lg) - 1u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t i = i0 + j;
        a.in[j] = i >= 0 && (uint32_t)i < extent;
        a.up[j] = a.in[j] && ((uint32_t)i >> lg) != a.lo;
        a.off[j] = a.in[j] ? (uint32_t)i & mask : 0u;
    }
}

// the lookup on a grid whose form is known at compile time: straight-line code, so that the 64 loads of a step are in flight together
template <bool dense>
VR_HD void cubic_lookup_form(const GridView& g, v3 ip, float& raw, v3& grad) {
    const uint32_t lg = dense ? 2u : 3u;
    CubicAxis X, Y, Z;
    cubic_axis(ip.x, dense ? (uint32_t)g.dim[0] : (uint32_t)g.nb[0] << 3, lg, X);
    cubic_axis(ip.y, dense ? (uint32_t)g.dim[1] : (uint32_t)g.nb[1] << 3, lg, Y);
    cubic_axis(ip.z, dense ? (uint32_t)g.dim[2] : (uint32_t)g.nb[2] << 3, lg, Z);
    const uint32_t nx = dense ? (uint32_t)g.dblk[0] : (uint32_t)g.nb[0], ny = dense ? (uint32_t)g.dblk[1] : (uint32_t)g.nb[1];
    // the 2 x 2 x 2 cells, [z][y][x]: index and decode range
    uint32_t cell[8];
    float rmin[8], rdiff[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t cz = (c & 4) ? Z.hi : Z.lo, cy = (c & 2) ? Y.hi : Y.lo, cx = (c & 1) ? X.hi : X.lo;
        cell[c] = (mul24(cz, ny) + cy) * nx + cx;
        rmin[c] = 0.0f; rdiff[c] = 0.0f;
        if (!dense) {
#if VR_BRICK_HEADERS
            const float* rec = reinterpret_cast<const float*>(g.atlas + (size_t)cell[c] * kBrickBlockBytes);      // line 0 of the block: every line repeats the range
#else
            const float* rec = g.rng + 2u * (size_t)cell[c];
#endif
            rmin[c] = rec[0]; rdiff[c] = rec[1];
        }
    }
    float s[4], sx[4], sy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the slab's four cells, then the row's two
        const uint32_t pc[4] = { Z.up[k] ? cell[4] : cell[0], Z.up[k] ? cell[5] : cell[1], Z.up[k] ? cell[6] : cell[2], Z.up[k] ? cell[7] : cell[3] };
        const float pm[4] = { Z.up[k] ? rmin[4] : rmin[0], Z.up[k] ? rmin[5] : rmin[1], Z.up[k] ? rmin[6] : rmin[2], Z.up[k] ? rmin[7] : rmin[3] };
        const float pd[4] = { Z.up[k] ? rdiff[4] : rdiff[0], Z.up[k] ? rdiff[5] : rdiff[1], Z.up[k] ? rdiff[6] : rdiff[2], Z.up[k] ? rdiff[7] : rdiff[3] };
        float r[4], rx[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t rc[2] = { Y.up[j] ? pc[2] : pc[0], Y.up[j] ? pc[3] : pc[1] };
            const float rm[2] = { Y.up[j] ? pm[2] : pm[0], Y.up[j] ? pm[3] : pm[1] };
            const float rd[2] = { Y.up[j] ? pd[2] : pd[0], Y.up[j] ? pd[3] : pd[1] };
            const bool in_zy = Z.in[k] & Y.in[j];
            const uint32_t off_zy = dense ? (Z.off[k] << 4) | (Y.off[j] << 2) : (Z.off[k] << 6) | (Y.off[j] << 3);
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t ct = X.up[i] ? rc[1] : rc[0], off = off_zy | X.off[i];
                VR_TRACE(1, g.atlas ? (const void*)g.atlas : (const void*)g.dense, ct, off);
                float val;
                if (dense) val = half2float(g.dense[(size_t)ct * 64u + off]);
                else {
#if VR_BRICK_HEADERS
                    const uint32_t b = g.atlas[(size_t)ct * kBrickBlockBytes + brick_voxel_byte(off)];
#else
                    const uint32_t b = g.atlas[(size_t)ct * 512u + off];
#endif
                    val = (X.up[i] ? rm[1] : rm[0]) + unorm8(b) * (X.up[i] ? rd[1] : rd[0]);
                }
                v[i] = (in_zy & X.in[i]) ? val : 0.0f;
            }
            r[j] = cubic_dot4(X.w, v[0], v[1], v[2], v[3]);
            rx[j] = cubic_dot4(X.d, v[0], v[1], v[2], v[3]);
        }
        s[k] = cubic_dot4(Y.w, r[0], r[1], r[2], r[3]);
        sx[k] = cubic_dot4(Y.w, rx[0], rx[1], rx[2], rx[3]);
        sy[k] = cubic_dot4(Y.d, r[0], r[1], r[2], r[3]);
    }
    raw = cubic_dot4(Z.w, s[0], s[1], s[2], s[3]);
    grad.x = cubic_dot4(Z.w, sx[0], sx[1], sx[2], sx[3]);
    grad.y = cubic_dot4(Z.w, sy[0], sy[1], sy[2], sy[3]);
    grad.z = cubic_dot4(Z.d, s[0], s[1], s[2], s[3]);
}
// raw value and gradient (voxel units) of the cubic B-spline field of grid g at index-space point ip; DENSE = 2: the grid's form is read from the view, once
template <int DENSE = 2>
VR_HD void cubic_lookup(const GridView& g, v3 ip, float& raw, v3& grad) {
    if (grid_is_dense<DENSE>(g)) cubic_lookup_form<true>(g, ip, raw, grad);
    else cubic_lookup_form<false>(g, ip, raw, grad);
}

}  // namespace vr
