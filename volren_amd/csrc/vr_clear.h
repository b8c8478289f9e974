// vr_clear.h -- the clear-distance table of a density grid: per cell of 8^3 voxels, how far the nearest cell lies in which a trilinear lookup could read
// anything but +0.  What the expected-value march (vr_expected.h) skips empty space by.
//
// The table, operation by operation (this text is the specification; tests/test_expected_skip_host.py restates it in numpy):
//   Cells     brick grids: the bricks, nb[0] x nb[1] x nb[2]; dense grids: ceil(dim / 8) cells per axis.  x fastest, one byte per cell; cells beyond the
//             grid do not exist in the table.
//   Voxels    a voxel inside the grid decodes as the taps decode it (vr_trace.h tap_value; the float of atlas_f32 where the view has one -- the same
//             number, decoded once): rmin + unorm8(b) * rdiff for bricks, the fp16 voxel for dense grids.  A voxel outside the grid is +0.
//   Clear     cell (cx, cy, cz) is clear when every voxel of [8 cx - 1, 8 cx + 8] x [8 cy - 1, 8 cy + 8] x [8 cz - 1, 8 cz + 8] -- its box grown by one
//             voxel on each side, 10^3 voxels -- has the bit pattern of +0.0f.  -0 and NaN are not +0.  The eight corners of a trilinear lookup at a
//             point of the cell, floor(p - 0.5) and one more per axis, lie in that box.
//   Reach     the table above has reach 1, what a trilinear lookup reads.  The table of reach 2 grows the box by two voxels on each side instead,
//             [8 c - 2, 8 c + 9] per axis, 12^3 voxels: what the 64 taps of the cubic lookup (vr_cubic.h: floor(p - 0.5) - 1 .. + 2 per axis) read at a
//             point of the cell.  Everything else is the same text; a grid keeps one table per reach.
//   Distance  d = min(255, max(|dx|, |dy|, |dz|) to the nearest cell that is not clear): 0 for a cell that is not clear, 255 for a grid without one.
// Built in two stages: the marking pass writes 0 or 255 per cell (clear_box_bits over the box), then one pass per axis replaces each byte by
// min over the cells c' of its row along that axis of max(|c - c'|, byte(c')) (clear_axis_pass): max distributes over min, and so does the cap.
#pragma once

#include "vr_trace.h"

namespace vr {

constexpr uint32_t kClearMax = 255u;
constexpr int32_t kClearBoxVoxels = 1000;           // 10^3: reach 1
constexpr int32_t kClearReaches = 2;                // reach 1 (trilinear) and 2 (cubic)

// (ClearTable, what the march gets, and clear_cells, the table's extent: vr_scene.h)

// the bits of voxel (x, y, z) as a tap decodes it; +0 outside the grid
VR_HD uint32_t clear_voxel_bits(const GridView& g, int32_t x, int32_t y, int32_t z) {
    const TapAddr a = tap_addr(g, x, y, z);
    if (!a.in) return 0u;
    if (!g.dense && g.atlas_f32) return f2u(g.atlas_f32[(size_t)a.cell * 512u + a.off]);
    return f2u(tap_value(g, tap_load(g, a), true));
}
// the OR of the bits of voxels first, first + stride, ... (< (8 + 2 reach)^3, x fastest) of the box of cell (cx, cy, cz) grown by `reach` voxels (1 or 2): 0 over
// the whole box = clear
VR_HD uint32_t clear_box_bits(const GridView& g, int32_t cx, int32_t cy, int32_t cz, int32_t first, int32_t stride, int32_t reach = 1) {
    const int32_t side = 8 + 2 * reach, slab = side * side;
    uint32_t acc = 0u;
    for (int32_t i = first; i < slab * side; i += stride) {
        const int32_t k = i / slab, j = (i - slab * k) / side;
        acc |= clear_voxel_bits(g, 8 * cx - reach + (i - slab * k - side * j), 8 * cy - reach + j, 8 * cz - reach + k);
    }
    return acc;
}
// one axis of the distance stage for cell (cx, cy, cz) of a table of n cells: a cell r away along the axis offers max(r, its byte) >= r, so the walk
// ends where r reaches the best offer so far
VR_HD uint32_t clear_axis_pass(const uint8_t* in, const int32_t n[3], int32_t axis, int32_t cx, int32_t cy, int32_t cz) {
    const size_t at = ((size_t)cz * (size_t)n[1] + (size_t)cy) * (size_t)n[0] + (size_t)cx;
    const size_t pitch = axis == 0 ? (size_t)1 : (axis == 1 ? (size_t)n[0] : (size_t)n[0] * (size_t)n[1]);
    const int32_t p = axis == 0 ? cx : (axis == 1 ? cy : cz), len = n[axis];
    uint32_t best = in[at];
    for (int32_t r = 1; (uint32_t)r < best; ++r) {
        if (p - r >= 0) { const uint32_t v = in[at - (size_t)r * pitch], o = v > (uint32_t)r ? v : (uint32_t)r; best = o < best ? o : best; }
        if (p + r < len) { const uint32_t v = in[at + (size_t)r * pitch], o = v > (uint32_t)r ? v : (uint32_t)r; best = o < best ? o : best; }
    }
    return best;
}

}  // namespace vr
