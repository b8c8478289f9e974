// vr_sky_tiles.h -- which 16x16 tiles of a frame no camera ray can hit the volume's box from (plain C++, host only; no HIP).
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

// the box as the camera sees it: the separating-axis candidates with the hull's extent along each.  valid = false: no tile is clear (the fallback)
struct SkyProjection {
    bool valid = false;
    int n_axes = 0;
    double ax[30], ay[30], lo[30], hi[30];      // axis (ax, ay) in pixel coordinates; the projections' dot products with it span [lo, hi]
};

inline SkyProjection sky_project_box(const SceneParams& P) {
    SkyProjection S;
    const Uniforms& u = P.u;
    const double W = (double)u.resolution[0], H = (double)u.resolution[1], cz = (double)P.cam_z;
    if (!(W >= 1.0) || !(H >= 1.0) || !std::isfinite(cz) || cz == 0.0) return S;
    // cam_transform is column-major (vr_math.h mat3_mul: column j at [3j .. 3j + 2]); its inverse by the adjugate
    double m[9], inv[9];
    for (int i = 0; i < 9; ++i) { m[i] = (double)u.cam_transform[i]; if (!std::isfinite(m[i])) return S; }
    const double c00 = m[4] * m[8] - m[7] * m[5], c01 = m[7] * m[2] - m[1] * m[8], c02 = m[1] * m[5] - m[4] * m[2];
    const double det = m[0] * c00 + m[3] * c01 + m[6] * c02;
    if (!std::isfinite(det) || det == 0.0) return S;
    // inv[3 * col + row], column-major like m
    inv[0] = c00 / det; inv[1] = c01 / det; inv[2] = c02 / det;
    inv[3] = (m[6] * m[5] - m[3] * m[8]) / det; inv[4] = (m[0] * m[8] - m[6] * m[2]) / det; inv[5] = (m[3] * m[2] - m[0] * m[5]) / det;
    inv[6] = (m[3] * m[7] - m[6] * m[4]) / det; inv[7] = (m[6] * m[1] - m[0] * m[7]) / det; inv[8] = (m[0] * m[4] - m[3] * m[1]) / det;
    double bb[2][3], cam[3];
    bool inside = true;
    for (int i = 0; i < 3; ++i) {
        bb[0][i] = (double)u.vol_bb_min[i]; bb[1][i] = (double)u.vol_bb_max[i]; cam[i] = (double)u.cam_pos[i];
        if (!std::isfinite(bb[0][i]) || !std::isfinite(bb[1][i]) || !std::isfinite(cam[i]) || bb[0][i] > bb[1][i]) return S;
        inside = inside && cam[i] >= bb[0][i] && cam[i] <= bb[1][i];
    }
    if (inside) return S;
    double X[8], Y[8];
    for (int k = 0; k < 8; ++k) {
        const double v[3] = { bb[k & 1][0] - cam[0], bb[(k >> 1) & 1][1] - cam[1], bb[(k >> 2) & 1][2] - cam[2] };
        const double lx = inv[0] * v[0] + inv[3] * v[1] + inv[6] * v[2], ly = inv[1] * v[0] + inv[4] * v[1] + inv[7] * v[2], lz = inv[2] * v[0] + inv[5] * v[1] + inv[8] * v[2];
        const double depth = lz / cz * std::fabs(cz);      // along the viewing axis (0, 0, cam_z) / |cam_z|, positive in front
        const double dist = std::sqrt(lx * lx + ly * ly + lz * lz);
        if (!std::isfinite(depth) || !std::isfinite(dist) || !(depth > 0.0) || !(depth >= kSkyFrontMargin * dist)) return S;
        X[k] = 0.5 * W + H * lx * cz / lz;
        Y[k] = 0.5 * H + H * ly * cz / lz;
        if (!std::isfinite(X[k]) || !std::isfinite(Y[k])) return S;
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

// is `tile` (raster id in the W x H frame) clear: its pixel rectangle inside the frame, grown by kSkyPixelMargin, strictly apart from the hull along one axis
inline bool sky_tile_clear(const SkyProjection& S, int32_t W, int32_t H, int32_t tile) {
    if (!S.valid) return false;
    const int32_t nx = tiles_x(W), tx = tile % nx, ty = tile / nx;
    const double x0 = (double)(tx * 16) - kSkyPixelMargin, y0 = (double)(ty * 16) - kSkyPixelMargin;
    const double x1 = (double)(tx * 16 + 16 < W ? tx * 16 + 16 : W) + kSkyPixelMargin, y1 = (double)(ty * 16 + 16 < H ? ty * 16 + 16 : H) + kSkyPixelMargin;
    for (int i = 0; i < S.n_axes; ++i) {
        const double ax = S.ax[i], ay = S.ay[i];
        const double rlo = (ax >= 0.0 ? ax * x0 : ax * x1) + (ay >= 0.0 ? ay * y0 : ay * y1);
        const double rhi = (ax >= 0.0 ? ax * x1 : ax * x0) + (ay >= 0.0 ? ay * y1 : ay * y0);
        if (rhi < S.lo[i] || rlo > S.hi[i]) return true;
    }
    return false;
}

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

}  // namespace vr
