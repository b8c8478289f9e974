// vr_sky_tiles.h -- which 16x16 tiles of a frame no camera ray can hit the volume's box from, and which ones no camera ray can reach density from (plain C++,
// host only; no HIP).  The CLEAR class first; the SEE-THROUGH class, which builds on its camera, in the second half.
//
// A tile is CLEAR when no camera ray of any of its pixels, for any jitter, can hit vol_bb_min .. vol_bb_max.  Every sample of such a tile is a primary miss
// (vr_trace.h sky_sample): the renderer renders these tiles with one thread per pixel (vr_launch.hip sky_kernel) and keeps them out of the path scheduler.
//
// The test.  do_new (vr_trace.h) shoots pixel (px, py) with jitter (jx, jy) along cam_transform * (fx, fy, cam_z), fx = ((px + jx) - W/2) / H, fy = ((py + jy) - H/2) / H:
// in continuous pixel coordinates (x, y) = (px + jx, py + jy) the ray is the point (x, y) of the image plane.  A box corner C lies on the ray through
//   (X, Y) = (W/2 + H * lx * cam_z / lz,  H/2 + H * ly * cam_z / lz),   (lx, ly, lz) = cam_transform^-1 (C - cam_pos)
// (the inverse is formed here: the matrix is not assumed orthonormal), provided lz / cam_z > 0, i.e. the corner lies in front of the camera.  With all eight
// corners in front, the rays that meet the box -- a convex body the camera is outside of -- are exactly the points of the convex hull of the eight projections.
// So a tile is clear when its pixel rectangle is disjoint from that hull: two convex polygons, decided by separating axes -- the rectangle's two, and the
// normal of the line through every pair of projections (the hull's edges are among those 28 lines).  All of it in double.
//
// The margin.  Jitter stays inside the closed pixel rectangle: rng (vr_math.h) returns k * 2^-24, k < 2^24, so px <= px + jx <= px + 1 also after rounding to
// float.  What the device computes differently from the exact geometry above is float rounding only: fx, fy, two normalisations, a 3x3 product and
// intersect_box's slabs, a few operations of relative error 2^-24 each -- some 1e-6 of the ray's direction, where one pixel is about 1e-3 rad (1 / H of the
// image plane's height, H of a few thousand at most).  The rectangle is therefore GROWN BY ONE WHOLE PIXEL on every side before the test: three orders of
// magnitude more than the rounding can move a ray, at the cost of the few tiles whose distance to the hull is below a pixel.
//
// The fallback.  NO tile is clear when a corner lies behind the camera or within kSkyFrontMargin of its plane (the projection is meaningless there, and
// unbounded near it), when the camera is inside the box, or when anything that enters the test is not finite.
//
// tests/hostkernel/sky_host.cpp builds this header for the host; tests/test_sky_tiles_host.py holds it to a lattice of slab tests and to the oracle.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "vr_scene.h"
#include "vr_tiles.h"

namespace vr {

// a corner counts as in front of the camera when its depth along the viewing axis is at least this share of its distance from the camera (0.06 degrees above the
// camera plane): far more than the float rounding of the depth, and it bounds the projections to 1000 image heights
constexpr double kSkyFrontMargin = 1e-3;
constexpr double kSkyPixelMargin = 1.0;      // whole pixels the tile's rectangle is grown by on every side (see above)

// the camera as the tests below take it, in double: frame size, cam_z, the camera's position and the inverse of cam_transform.  valid = false: nothing is decided
struct SkyCamera {
    bool valid = false;
    double W = 0.0, H = 0.0, cz = 0.0, inv[9], cam[3];
};

inline SkyCamera sky_camera(const SceneParams& P) {
    SkyCamera C;
    const Uniforms& u = P.u;
    const double W = (double)u.resolution[0], H = (double)u.resolution[1], cz = (double)P.cam_z;
    if (!(W >= 1.0) || !(H >= 1.0) || !std::isfinite(cz) || cz == 0.0) return C;
    // cam_transform is column-major (vr_math.h mat3_mul: column j at [3j .. 3j + 2]); its inverse by the adjugate
    double m[9];
    double* inv = C.inv;
    for (int i = 0; i < 9; ++i) { m[i] = (double)u.cam_transform[i]; if (!std::isfinite(m[i])) return C; }
    const double c00 = m[4] * m[8] - m[7] * m[5], c01 = m[7] * m[2] - m[1] * m[8], c02 = m[1] * m[5] - m[4] * m[2];
    const double det = m[0] * c00 + m[3] * c01 + m[6] * c02;
    if (!std::isfinite(det) || det == 0.0) return C;
    // inv[3 * col + row], column-major like m
    inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
    inv[3] = (m[6] * m[5] - m[3] * m[8]) / det; inv[4] = (m[0] * m[8] - m[6] * m[2]) / det; inv[5] = (m[3] * m[2] - m[0] * m[5]) / det;
    inv[6] = (m[3] * m[7] - m[6] * m[4]) / det; inv[7] = (m[6] * m[1] - m[0] * m[7]) / det; inv[8] = (m[0] * m[4] - m[3] * m[1]) / det;
    for (int i = 0; i < 3; ++i) { C.cam[i] = (double)u.cam_pos[i]; if (!std::isfinite(C.cam[i])) return C; }
    C.W = W; C.H = H; C.cz = cz;
    C.valid = true;
    return C;
}

// the point (X, Y) of the image plane, in continuous pixel coordinates, whose ray passes through the world-space point c.  false: c lies behind the camera or within
// kSkyFrontMargin of its plane, or something is not finite -- the caller falls back
inline bool sky_project_point(const SkyCamera& C, const double c[3], double& X, double& Y) {
    const double* inv = C.inv;
    const double v[3] = { c[0] - C.cam[0], c[1] - C.cam[1], c[2] - C.cam[2] };
    const double lx = inv[0] * v[0] + inv[3] * v[1] + inv[6] * v[2], ly = inv[1] * v[0] + inv[4] * v[1] + inv[7] * v[2], lz = inv[2] * v[0] + inv[5] * v[1] + inv[8] * v[2];
    const double depth = lz / C.cz * std::fabs(C.cz);      // along the viewing axis (0, 0, cam_z) / |cam_z|, positive in front
    const double dist = std::sqrt(lx * lx + ly * ly + lz * lz);
    if (!std::isfinite(depth) || !std::isfinite(dist) || !(depth > 0.0) || !(depth >= kSkyFrontMargin * dist)) return false;
    X = 0.5 * C.W + C.H * lx * C.cz / lz;
    Y = 0.5 * C.H + C.H * ly * C.cz / lz;
    return std::isfinite(X) && std::isfinite(Y);
}

// the box as the camera sees it: the separating-axis candidates with the hull's extent along each.  valid = false: no tile is clear (the fallback)
struct SkyProjection {
    bool valid = false;
    int n_axes = 0;
    double ax[30], ay[30], lo[30], hi[30];      // axis (ax, ay) in pixel coordinates; the projections' dot products with it span [lo, hi]
};

// the camera lies inside the (closed) box vol_bb_min .. vol_bb_max; also true when the box is not a finite, ordered one
inline bool sky_camera_in_box(const SkyCamera& C, const Uniforms& u, double bb[2][3]) {
    bool inside = true;
    for (int i = 0; i < 3; ++i) {
        bb[0][i] = (double)u.vol_bb_min[i]; bb[1][i] = (double)u.vol_bb_max[i];
        if (!std::isfinite(bb[0][i]) || !std::isfinite(bb[1][i]) || bb[0][i] > bb[1][i]) return true;
        inside = inside && C.cam[i] >= bb[0][i] && C.cam[i] <= bb[1][i];
    }
    return inside;
}

inline SkyProjection sky_project_box(const SceneParams& P) {
    SkyProjection S;
    const SkyCamera C = sky_camera(P);
    if (!C.valid) return S;
    double bb[2][3];
    if (sky_camera_in_box(C, P.u, bb)) return S;
    double X[8], Y[8];
    for (int k = 0; k < 8; ++k) {
        const double c[3] = { bb[k & 1][0], bb[(k >> 1) & 1][1], bb[(k >> 2) & 1][2] };
        if (!sky_project_point(C, c, X[k], Y[k])) return S;
    }
    auto add_axis = [&](double ax, double ay) {
        if (ax == 0.0 && ay == 0.0) return;                // two projections coincide: no line
        double lo = ax * X[0] + ay * Y[0], hi = lo;
        for (int k = 1; k < 8; ++k) { const double d = ax * X[k] + ay * Y[k]; lo = d < lo ? d : lo; hi = d > hi ? d : hi; }
        S.ax[S.n_axes] = ax; S.ay[S.n_axes] = ay; S.lo[S.n_axes] = lo; S.hi[S.n_axes] = hi;
        ++S.n_axes;
    };
    add_axis(1.0, 0.0);
    add_axis(0.0, 1.0);
    for (int a = 0; a < 8; ++a)
        for (int b = a + 1; b < 8; ++b) {
            // unit normal of the line through projections a and b (the length only scales both intervals; normalised so that no product overflows)
            const double ex = X[b] - X[a], ey = Y[b] - Y[a], len = std::sqrt(ex * ex + ey * ey);
            if (len > 0.0 && std::isfinite(len)) add_axis(-ey / len, ex / len);
        }
    S.valid = true;
    return S;
}

// is the pixel rectangle of `tile` (raster id in the W x H frame) inside the frame, grown by `margin` pixels on every side (shrunk by a negative one), strictly
// apart from the hull along one axis.  The axes are the rectangle's and the normals of the hull's edges, so for two convex polygons "apart along none" is "they meet"
inline bool sky_tile_apart(const SkyProjection& S, int32_t W, int32_t H, int32_t tile, double margin) {
    if (!S.valid) return false;
    const int32_t nx = tiles_x(W), tx = tile % nx, ty = tile / nx;
    const double x0 = (double)(tx * 16) - margin, y0 = (double)(ty * 16) - margin;
    const double x1 = (double)(tx * 16 + 16 < W ? tx * 16 + 16 : W) + margin, y1 = (double)(ty * 16 + 16 < H ? ty * 16 + 16 : H) + margin;
    if (x0 > x1 || y0 > y1) return true;                  // a ragged tile thinner than twice the (negative) margin: nothing left of it
    for (int i = 0; i < S.n_axes; ++i) {
        const double ax = S.ax[i], ay = S.ay[i];
        const double rlo = (ax >= 0.0 ? ax * x0 : ax * x1) + (ay >= 0.0 ? ay * y0 : ay * y1);
        const double rhi = (ax >= 0.0 ? ax * x1 : ax * x0) + (ay >= 0.0 ? ay * y1 : ay * y0);
        if (rhi < S.lo[i] || rlo > S.hi[i]) return true;
    }
    return false;
}
// is `tile` clear: its rectangle grown by kSkyPixelMargin lies apart from the hull
inline bool sky_tile_clear(const SkyProjection& S, int32_t W, int32_t H, int32_t tile) { return sky_tile_apart(S, W, H, tile, kSkyPixelMargin); }
// do rays of `tile` surely cross the box: its rectangle SHRUNK by kSkyPixelMargin still meets the hull.  The tiles that are neither clear nor crossed -- the ring
// along the box's silhouette that the margin leaves undecided either way -- belong to no class and stay with the path tracer
inline bool sky_tile_crossed(const SkyProjection& S, int32_t W, int32_t H, int32_t tile) { return S.valid && !sky_tile_apart(S, W, H, tile, -kSkyPixelMargin); }

// clear[i] = 1 when tiles[i] is clear, else 0
inline void sky_classify_tiles(const SceneParams& P, const int32_t* tiles, int32_t n, uint8_t* clear) {
    const SkyProjection S = sky_project_box(P);
    for (int32_t i = 0; i < n; ++i) clear[i] = sky_tile_clear(S, P.u.resolution[0], P.u.resolution[1], tiles[i]) ? 1 : 0;
}

// The one split of a tile list: `ids` (empty = the n_tiles tiles of the whole frame, in raster order) into the tiles the path tracer marches and the clear
// ones, each in the order of `ids`.
inline void sky_split_tiles(const SceneParams& P, const std::vector<int32_t>& ids, int32_t n_tiles, std::vector<int32_t>& march, std::vector<int32_t>& sky) {
    march.clear(); sky.clear();
    const SkyProjection S = sky_project_box(P);
    const int32_t n = ids.empty() ? n_tiles : (int32_t)ids.size();
    for (int32_t i = 0; i < n; ++i) {
        const int32_t t = ids.empty() ? i : ids[(size_t)i];
        (sky_tile_clear(S, P.u.resolution[0], P.u.resolution[1], t) ? sky : march).push_back(t);
    }
}

// ---- see-through tiles ---------------------------------------------------------------------------------------------------------------------------------
//
// A tile is SEE-THROUGH when rays of it surely cross the box (sky_tile_crossed: its rectangle shrunk by the pixel margin meets the box's projection -- so it is not
// clear, and not one of the silhouette's ring of tiles that are merely not clear by the margin) and no camera ray of its pixels, for any jitter, passes within tap
// reach of a LIVE cell of the density grid: its rays cross the box, but nothing they can read there has density > 0.  Every sample of such a tile is the sky's as well -- (show_environment ?
// lookup_environment(dir) : 0, alpha 0), what sky_sample writes -- and the renderer renders these tiles beside the clear ones (sky_kernel, without the box test).
//
// Why that is exact.  For integrators 0 and 1, without an emission grid and without a transfer function, a camera sample's output depends on its camera segment
// only through "did a real collision happen": if none did, trace_path leaves its loop with n_paths == 0, L = 0, throughput 1 and mis = 1, and the escape writes
// L + (1 * 1) * Le with alpha 0; the draws the segment consumed are never used again, because the sample ends there.  A real collision needs
// rng * majorant < d (the DDA tracker) or rng < d * inv_majorant (the global tracker), d = density_scale * (the voxel a tap read): with density_scale >= 0 and
// every voxel a tap can read decoding to <= 0, d <= 0 (or NaN) while the left side is >= 0 (or NaN), and neither comparison can hold.  Tentative collisions
// that the coarse majorant levels produce over empty cells are NULL collisions: they draw, compare false and change nothing the result sees.  A free-flight draw
// of exactly 0 in an empty cell (majorant 0) makes the ray parameter 0 / 0 = NaN: every fetch then reads "outside" (vr_trace.h, the comment at nan_guard), the
// collision is null, and the loop ends -- no hit either.
//
// Live cells.  The density grid's range table has one fp16 (min, max) word per cell of 8^3 voxels (BrickGrid::range, DenseGridF16::range; a brick's voxels decode
// to rmin + u8 / 255 * (max - min), inside [min, max]; a dense grid's cell range covers its voxels and two more on every side).  A cell is DEAD when both halves
// are finite and <= 0, LIVE otherwise.  SkyLiveCells is a pyramid of "some cell below is live" over the level-0 words, built once per committed grid
// (sky_live_cells).  It is built from the level-0 words and not read from the grid's own range mips: those keep the largest maximum and so drop a NaN child, and a
// .brick file's mips are whatever the file holds.  A NaN half anywhere gives no see-through tile at all.
//
// Tap reach.  tricubic_tap_t (vr_trace.h) reads voxel floor(p - 0.5) + j - 1, j = 0 .. 3, per axis: with floor(p - 0.5) in (p - 1.5, p - 0.5] the voxels read
// span (p - 2.5, p + 2.5] -- a point reads a voxel of cell [8 c, 8 c + 8] only from within kSkyTapReach = 2.5 voxels of it (the trilinear lookup reaches less).
// A live cell's index-space box is grown by that reach PLUS ONE WHOLE VOXEL (the float rounding of the index-space ray, some 1e-4 voxels on a grid of a thousand,
// with four orders of magnitude to spare), its eight corners go through vol_density_transform to the image plane, and their bounding rectangle is grown by
// kSkyPixelMargin like a clear tile's.  Every tile that rectangle touches is marked; the unmarked ones whose rays surely cross the box (sky_tile_crossed) are see-through.  The clip planes only
// shorten the segment, so ignoring them is conservative.
//
// The descent starts at the pyramid's top.  A cell with no live cell below it is skipped whole; a cell whose rectangle lies in one tile, or whose tiles are all
// marked already, marks and stops; the others descend.  So the cost goes by the tiles, not by the bricks.
//
// Fallbacks: NO see-through tile when a grown live cell has a corner behind the camera or within kSkyFrontMargin of its plane (at level 0; coarser cells descend
// instead), when the camera is inside the box, when an emission grid or a transfer function is bound, when the density scale is not finite and >= 0, when the
// integrator is not 0 or 1, when the host holds no range table for the grid (a grid encoded on the device), or when a range half is NaN.
//
// tests/hostkernel/see_through_host.cpp builds this for the host; tests/test_see_through_host.py holds it to a lattice of slab tests against the grown live
// bricks and to the oracle.
constexpr double kSkyTapReach = 2.5;                      // voxels between a point and the farthest face of a voxel its tap can read (derived above)
constexpr double kSkyCellGrow = kSkyTapReach + 1.0;       // what a live cell's index-space box is grown by

// a range half that cannot make a voxel decode above 0: finite and <= 0 (either zero, or negative)
inline bool sky_half_dead(uint32_t h) { h &= 0xFFFFu; return (h & 0x7FFFu) == 0u || ((h & 0x8000u) != 0u && (h & 0x7C00u) != 0x7C00u); }
inline bool sky_half_nan(uint32_t h) { return (h & 0x7C00u) == 0x7C00u && (h & 0x03FFu) != 0u; }

struct SkyLiveCells {
    bool held = false;                                    // the host holds the grid's range table (false: no see-through tile)
    bool nan = false;                                     // a range half is NaN (no see-through tile)
    std::vector<std::vector<uint8_t>> live;               // level m: 1 = a level-0 cell below cell (x, y, z) of (8 << m)^3 voxels is live; x fastest
    std::vector<int32_t> n;                               // 3 per level: cells per axis, ceil(n of level 0 / 2^m); the last level is one cell
};

// range: nx * ny * nz words, x fastest, low half = min, high half = max
inline SkyLiveCells sky_live_cells(const uint32_t* range, int32_t nx, int32_t ny, int32_t nz) {
    SkyLiveCells L;
    if (!range || nx <= 0 || ny <= 0 || nz <= 0) return L;
    L.held = true;
    const size_t n0 = (size_t)nx * (size_t)ny * (size_t)nz;
    L.live.emplace_back(n0);
    L.n = { nx, ny, nz };
    for (size_t i = 0; i < n0; ++i) {
        const uint32_t w = range[i];
        L.nan = L.nan || sky_half_nan(w) || sky_half_nan(w >> 16);
        L.live[0][i] = (sky_half_dead(w) && sky_half_dead(w >> 16)) ? 0 : 1;
    }
    for (size_t m = 0; L.n[3 * m] > 1 || L.n[3 * m + 1] > 1 || L.n[3 * m + 2] > 1; ++m) {
        const int32_t sx = L.n[3 * m], sy = L.n[3 * m + 1], sz = L.n[3 * m + 2];
        const int32_t dx = (sx + 1) / 2, dy = (sy + 1) / 2, dz = (sz + 1) / 2;
        std::vector<uint8_t> dst((size_t)dx * (size_t)dy * (size_t)dz, 0);
        const std::vector<uint8_t>& src = L.live[m];
        for (int32_t z = 0; z < sz; ++z)
            for (int32_t y = 0; y < sy; ++y)
                for (int32_t x = 0; x < sx; ++x)
                    if (src[((size_t)z * sy + y) * sx + x]) dst[((size_t)(z >> 1) * dy + (y >> 1)) * dx + (x >> 1)] = 1;
        L.live.push_back(std::move(dst));
        L.n.push_back(dx); L.n.push_back(dy); L.n.push_back(dz);
    }
    return L;
}

// what the uniforms say about the see-through class: the fallbacks that need neither camera nor grid
inline bool sky_see_through_scene(const Uniforms& u) {
    return (u.integrator == 0 || u.integrator == 1) && u.has_emission == 0 && u.use_tf == 0 && std::isfinite(u.vol_density_scale) && u.vol_density_scale >= 0.0f;
}

// The tiles of the frame that a camera ray can reach a live cell from.  valid = false: the fallback, no see-through tile.
struct SkyTouched {
    bool valid = false;
    int32_t nx = 0, ny = 0;
    std::vector<uint8_t> tile;                            // nx * ny, raster: 1 = a grown live cell's rectangle touches the tile
    int64_t cells_visited = 0;                            // pyramid cells the descent looked at (the tests bound it)
};

inline SkyTouched sky_touched_tiles(const SceneParams& P, const SkyLiveCells& L) {
    SkyTouched T;
    const Uniforms& u = P.u;
    if (!L.held || L.nan || !sky_see_through_scene(u)) return T;
    const SkyCamera C = sky_camera(P);
    if (!C.valid) return T;
    double bb[2][3];
    if (sky_camera_in_box(C, u, bb)) return T;
    double xf[16];
    for (int i = 0; i < 16; ++i) { xf[i] = (double)u.vol_density_transform[i]; if (!std::isfinite(xf[i])) return T; }
    T.nx = tiles_x(u.resolution[0]); T.ny = tiles_y(u.resolution[1]);
    T.tile.assign((size_t)T.nx * (size_t)T.ny, 0);
    struct Cell { int32_t m, x, y, z; };
    std::vector<Cell> stack;
    const int32_t top = (int32_t)L.live.size() - 1;
    stack.push_back(Cell{ top, 0, 0, 0 });
    while (!stack.empty()) {
        const Cell c = stack.back();
        stack.pop_back();
        const int32_t sx = L.n[3 * (size_t)c.m], sy = L.n[3 * (size_t)c.m + 1];
        ++T.cells_visited;
        if (!L.live[(size_t)c.m][((size_t)c.z * sy + c.y) * sx + c.x]) continue;
        const double s = (double)(8 << c.m);
        const double lo[3] = { c.x * s - kSkyCellGrow, c.y * s - kSkyCellGrow, c.z * s - kSkyCellGrow };
        const double hi[3] = { (c.x + 1) * s + kSkyCellGrow, (c.y + 1) * s + kSkyCellGrow, (c.z + 1) * s + kSkyCellGrow };
        bool front = true;
        double X0 = 0.0, X1 = 0.0, Y0 = 0.0, Y1 = 0.0;
        for (int k = 0; k < 8 && front; ++k) {
            const double ip[3] = { (k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2] };
            double w[3], X, Y;                            // index space -> world: vol_density_transform, column-major (vr_math.h mat4_point)
            for (int r = 0; r < 3; ++r) w[r] = xf[r] * ip[0] + xf[4 + r] * ip[1] + xf[8 + r] * ip[2] + xf[12 + r];
            front = sky_project_point(C, w, X, Y);
            if (!front) break;
            if (k == 0) { X0 = X1 = X; Y0 = Y1 = Y; }
            else { X0 = X < X0 ? X : X0; X1 = X > X1 ? X : X1; Y0 = Y < Y0 ? Y : Y0; Y1 = Y > Y1 ? Y : Y1; }
        }
        bool descend = !front;
        if (!front && c.m == 0) return SkyTouched{};       // a live cell the projection says nothing about: the fallback
        if (front) {
            // tiles the closed rectangle [X0 - margin, X1 + margin] x [Y0 - margin, Y1 + margin] touches; tile t covers [16 t, 16 t + 16], closed as well
            const double fx0 = std::ceil((X0 - kSkyPixelMargin) / 16.0) - 1.0, fx1 = std::floor((X1 + kSkyPixelMargin) / 16.0);
            const double fy0 = std::ceil((Y0 - kSkyPixelMargin) / 16.0) - 1.0, fy1 = std::floor((Y1 + kSkyPixelMargin) / 16.0);
            if (fx1 < 0.0 || fy1 < 0.0 || fx0 > (double)(T.nx - 1) || fy0 > (double)(T.ny - 1)) continue;      // beside the frame
            const int32_t tx0 = fx0 < 0.0 ? 0 : (int32_t)fx0, tx1 = fx1 > (double)(T.nx - 1) ? T.nx - 1 : (int32_t)fx1;
            const int32_t ty0 = fy0 < 0.0 ? 0 : (int32_t)fy0, ty1 = fy1 > (double)(T.ny - 1) ? T.ny - 1 : (int32_t)fy1;
            bool all_marked = true;
            for (int32_t ty = ty0; ty <= ty1 && all_marked; ++ty)
                for (int32_t tx = tx0; tx <= tx1; ++tx)
                    if (!T.tile[(size_t)ty * T.nx + tx]) { all_marked = false; break; }
            if (all_marked) continue;
            if (c.m == 0 || (tx0 == tx1 && ty0 == ty1)) {
                for (int32_t ty = ty0; ty <= ty1; ++ty)
                    for (int32_t tx = tx0; tx <= tx1; ++tx) T.tile[(size_t)ty * T.nx + tx] = 1;
                continue;
            }
            descend = true;
        }
        if (descend) {
            const int32_t cx = L.n[3 * (size_t)(c.m - 1)], cy = L.n[3 * (size_t)(c.m - 1) + 1], cz = L.n[3 * (size_t)(c.m - 1) + 2];
            for (int k = 0; k < 8; ++k) {
                const int32_t x = 2 * c.x + (k & 1), y = 2 * c.y + ((k >> 1) & 1), z = 2 * c.z + (k >> 2);
                if (x < cx && y < cy && z < cz) stack.push_back(Cell{ c.m - 1, x, y, z });
            }
        }
    }
    T.valid = true;
    return T;
}

// cls[i] of tiles[i]: 0 march, 1 clear, 2 see-through
enum : uint8_t { kSkyMarch = 0, kSkyClear = 1, kSkySeeThrough = 2 };
inline void sky_classify_tiles3(const SceneParams& P, const SkyLiveCells& L, const int32_t* tiles, int32_t n, uint8_t* cls) {
    const SkyProjection S = sky_project_box(P);
    const SkyTouched T = S.valid ? sky_touched_tiles(P, L) : SkyTouched{};
    for (int32_t i = 0; i < n; ++i) {
        const int32_t t = tiles[i];
        if (sky_tile_clear(S, P.u.resolution[0], P.u.resolution[1], t)) cls[i] = kSkyClear;
        else cls[i] = (T.valid && t >= 0 && (size_t)t < T.tile.size() && !T.tile[(size_t)t] && sky_tile_crossed(S, P.u.resolution[0], P.u.resolution[1], t)) ? kSkySeeThrough : kSkyMarch;
    }
}

// The three-way split of a tile list: `ids` (empty = the n_tiles tiles of the whole frame, in raster order) into march, clear and see-through tiles, each in the
// order of `ids`.  march + see is sky_split_tiles' march list, clear its sky list.
inline void sky_split_tiles3(const SceneParams& P, const SkyLiveCells& L, const std::vector<int32_t>& ids, int32_t n_tiles, std::vector<int32_t>& march,
                             std::vector<int32_t>& clear, std::vector<int32_t>& see) {
    march.clear(); clear.clear(); see.clear();
    const int32_t n = ids.empty() ? n_tiles : (int32_t)ids.size();
    std::vector<int32_t> all;
    if (ids.empty()) { all.resize((size_t)n); for (int32_t i = 0; i < n; ++i) all[(size_t)i] = i; }
    const int32_t* t = ids.empty() ? all.data() : ids.data();
    std::vector<uint8_t> cls((size_t)n);
    sky_classify_tiles3(P, L, t, n, cls.data());
    for (int32_t i = 0; i < n; ++i) (cls[(size_t)i] == kSkyClear ? clear : cls[(size_t)i] == kSkySeeThrough ? see : march).push_back(t[i]);
}

}  // namespace vr
