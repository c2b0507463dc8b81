// raynet_overlap_args.h -- the argument checks, the launch geometry and the per-point predicates of
// rn_view_overlap / rn_view_gain (raynet_overlap.inl), host-only and free of HIP so that they
// compile into a stand-alone program (tests/overlap_args_main.cpp, built with the address and
// undefined-behaviour sanitizers by tests/test_view_selection_cpu.py).  The launchers act on the
// verdicts; the kernels decide whether a view sees a point (`sees`), whether two views share it
// (`shares`) and whether a point is short of views (`is_short`) with the constexpr functions below.
//
// Seeing is rn_view::observe's `ok` without the colour fetch: rn_view::project, the facing test on
// squares, the nearest pixel of the depth map.  Sharing is a band of the triangulation angle,
// decided on squared cosines as computed; no square root and no libm call anywhere, so that a NumPy
// restatement gives the same integers (tests/view_selection_truth.py).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_views_args.h"

namespace rn_overlap {

using rn_view::CAMERA_DOUBLES, rn_view::map_index, rn_view::pixel_in;

constexpr int MAX_VIEWS = 64;                       // one bit of the 64-bit mask each
constexpr int64_t MAX_POINTS = (int64_t)1 << 38;    // rejects garbage; bounds a block's counters
constexpr int BLOCK_SIZE = 256;                     // four wavefronts; one point per lane and tile
constexpr int MAX_BLOCKS = 1024;                    // four per CU of 256, whatever n is
constexpr int MAX_PAIRS = MAX_VIEWS * (MAX_VIEWS + 1) / 2;      // 2080 counters, 8320 bytes of LDS

enum Verdict { INVALID = -1, EMPTY = 0, LAUNCH = 1 };

// rn_view_overlap.  The scalars first, then n == 0 (nothing to write: EMPTY, whatever the
// pointers), then the pointers: points, cameras, visible and pairs always; normals and depths may
// be NULL (no facing test, no occlusion test).
inline Verdict overlap_args(bool have_ctx, int64_t n, const void *points, const void *normals,
                            int32_t V, const void *cameras, int32_t H, int32_t W,
                            const void *depths, double tol, double min_cos, double border,
                            double cos_lo, double cos_hi, const void *visible, const void *pairs) {
    (void)normals;
    (void)depths;
    if (!have_ctx || n < 0 || n > MAX_POINTS) return INVALID;
    if (V < 1 || V > MAX_VIEWS) return INVALID;
    if (H < 1 || W < 1) return INVALID;
    if (!(tol >= 0.0) || !std::isfinite(tol)) return INVALID;
    if (!(min_cos >= 0.0) || !std::isfinite(min_cos)) return INVALID;
    if (!(border >= 0.0) || !std::isfinite(border)) return INVALID;
    if (!(cos_lo >= 0.0) || !(cos_lo <= cos_hi) || !(cos_hi <= 1.0)) return INVALID;
    if (n == 0) return EMPTY;
    if (!points || !cameras || !visible || !pairs) return INVALID;
    return LAUNCH;
}

// rn_view_gain.  chosen is a bit pattern: every value is accepted.
inline Verdict gain_args(bool have_ctx, int64_t n, const void *visible, int32_t V,
                         int32_t redundancy, const void *gain) {
    if (!have_ctx || n < 0 || n > MAX_POINTS) return INVALID;
    if (V < 1 || V > MAX_VIEWS) return INVALID;
    if (redundancy < 1 || redundancy > MAX_VIEWS) return INVALID;
    if (n == 0) return EMPTY;
    if (!visible || !gain) return INVALID;
    return LAUNCH;
}

// ---- the launch: tiles of BLOCK_SIZE points, at most MAX_BLOCKS blocks, block b takes the tiles
// b, b + blocks, b + 2 blocks, ... ----
constexpr int64_t tiles(int64_t n) { return (n + BLOCK_SIZE - 1) / BLOCK_SIZE; }
constexpr int64_t blocks(int64_t n) { return tiles(n) < MAX_BLOCKS ? tiles(n) : MAX_BLOCKS; }
constexpr bool point_in(int64_t i, int64_t n) { return i >= 0 && i < n; }
// the most points one block meets: what one of its uint32 counters can reach
constexpr int64_t block_points_max(int64_t n) {
    return blocks(n) > 0 ? ((tiles(n) + blocks(n) - 1) / blocks(n)) * BLOCK_SIZE : 0;
}
// the largest cloud: 2^30 tiles over 1024 blocks, 2^20 tiles of 256 points per block = 2^28 -- a
// block's uint32 counter cannot wrap; and below the block cap a block takes one tile
static_assert(block_points_max(MAX_POINTS) == ((int64_t)1 << 28), "counters: 2^28 per block");
static_assert(block_points_max(MAX_POINTS) < ((int64_t)1 << 32), "a uint32 counter would wrap");
static_assert(block_points_max((int64_t)MAX_BLOCKS * BLOCK_SIZE) == BLOCK_SIZE, "one tile each");
static_assert(MAX_PAIRS * sizeof(uint32_t) == 8320, "the LDS table");

// coordinate k of point i of a [3][n] table: three streams, each contiguous over the points
constexpr size_t coord_index(int k, int64_t i, int64_t n) {
    return (size_t)k * (size_t)n + (size_t)i;
}
// the counter of the pair i <= j among V views: the upper triangle row by row, the diagonal first
constexpr int pair_index(int i, int j, int V) { return i * V - i * (i - 1) / 2 + (j - i); }
constexpr int pair_count(int V) { return V * (V + 1) / 2; }
// entry (i, j) of the [V][V] matrix
constexpr size_t matrix_index(int i, int j, int V) { return (size_t)i * (size_t)V + (size_t)j; }
// the bits of the views 0 .. V - 1
constexpr uint64_t low_bits(int V) { return V >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << V) - 1); }

// ---- whether one view sees one point: rn_view::observe's ok.  nn = |normal|^2 (0: no facing
// test), mc2 = min_cos^2; depths NULL: no occlusion test.  Also the vector to the centre and its
// squared length, as project computed them.  Every test is a comparison that a NaN fails. ----
struct Sight {
    bool ok;
    double dx, dy, dz, dd;
};
__attribute__((always_inline)) constexpr Sight sees(const double *cameras, int v, double x,
                                                    double y, double z, double nx, double ny,
                                                    double nz, double nn, double mc2, int H, int W,
                                                    const float *depths, double tol, double border,
                                                    double x_max, double y_max) {
    const rn_view::Projection p = rn_view::project(cameras + CAMERA_DOUBLES * v, x, y, z, border,
                                                   x_max, y_max);
    bool ok = p.ok;
    if (nn > 0.0) {
        const double dot = (nx * p.dx + ny * p.dy) + nz * p.dz, q = nn * p.dd;
        const double dot2 = dot * dot;
        ok = ok && dot > 0.0 && dot2 > mc2 * q;
    }
    if (depths) {
        // a view that does not count reads pixel (0, 0): every load is inside the array
        const int xr = (int)std::rint(ok ? p.X : 0.0), yr = (int)std::rint(ok ? p.Y : 0.0);
        const float zf = depths[map_index(v, pixel_in(yr, H) ? yr : 0, pixel_in(xr, W) ? xr : 0,
                                          H, W)];
        const double lim = (double)zf + tol;
        ok = ok && zf > 0.0f && p.dd <= lim * lim;
    }
    return Sight{ok, p.dx, p.dy, p.dz, p.dd};
}

// the vector from a point to view v's centre and its squared length, with project's operations:
// the same bits
struct ToCentre {
    double dx, dy, dz, dd;
};
__attribute__((always_inline)) constexpr ToCentre to_centre(const double *cameras, int v, double x,
                                                            double y, double z) {
    const double *cam = cameras + CAMERA_DOUBLES * v;
    const double dx = cam[12] - x, dy = cam[13] - y, dz = cam[14] - z;
    return ToCentre{dx, dy, dz, (dx * dx + dy * dy) + dz * dz};
}

// ---- whether two views that both see a point share it: the cosine of the angle between the
// point's rays to the two centres lies in [cos_lo, cos_hi], decided on squares as computed ----
__attribute__((always_inline)) constexpr bool shares(const ToCentre &a, const ToCentre &b,
                                                     double lo2, double hi2) {
    const double dot = (a.dx * b.dx + a.dy * b.dy) + a.dz * b.dz;
    const double q = a.dd * b.dd;
    const double dot2 = dot * dot;
    return dot > 0.0 && dot2 >= lo2 * q && dot2 <= hi2 * q;
}

// ---- whether fewer than `redundancy` of the chosen views see a point ----
constexpr int popcount64(uint64_t m) { return __builtin_popcountll(m); }
constexpr bool is_short(uint64_t visible, uint64_t chosen, int V, int redundancy) {
    return popcount64(visible & chosen & low_bits(V)) < redundancy;
}

}  // namespace rn_overlap
