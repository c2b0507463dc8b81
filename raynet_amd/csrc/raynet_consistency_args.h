// raynet_consistency_args.h -- the argument checks and the index arithmetic of
// rn_points_consistency (raynet_consistency.inl), host-only and free of HIP so that they compile
// into a stand-alone program (tests/consistency_args_main.cpp, built with the address and
// undefined-behaviour sanitizers by tests/test_consistency_cpu.py).  The launcher acts on the
// verdict; the kernel finds its point and addresses the maps with the constexpr functions below,
// and classifies a view with `classify`.
//
// The signed distance is rn_tsdf_integrate's, s = (z z - dd) / (z + z) (raynet_fusion_args.h): zero
// exactly where the point lies at the recorded depth, positive in front of the recorded surface,
// and free of a square root, so that a NumPy restatement gives the same bits
// (tests/consistency_truth.py).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_views_args.h"

namespace rn_consistency {

using rn_view::CAMERA_DOUBLES, rn_view::map_index, rn_view::pixel_in;

constexpr int MAX_VIEWS = 32;                       // one bit of the three masks each
constexpr int64_t MAX_POINTS = (int64_t)1 << 38;    // rejects garbage; 2^30 blocks of 256

enum Verdict { INVALID = -1, EMPTY = 0, LAUNCH = 1 };

// rn_points_consistency.  The scalars first, then n == 0 (nothing to write: EMPTY, whatever the
// pointers), then the pointers.  There is always a view, so cameras and depths are always read.
inline Verdict points_args(bool have_ctx, int64_t n, const void *points, int32_t V,
                           const void *cameras, int32_t H, int32_t W, const void *depths,
                           int32_t exclude, double tol_abs, double tol_rel, double border,
                           const void *seen, const void *agree, const void *violate,
                           const void *residual) {
    if (!have_ctx || n < 0 || n > MAX_POINTS) return INVALID;
    if (V < 1 || V > MAX_VIEWS) return INVALID;
    if (H < 1 || W < 1) return INVALID;
    if (exclude < -1 || exclude >= V) return INVALID;
    if (!(tol_abs >= 0.0) || !std::isfinite(tol_abs)) return INVALID;
    if (!(tol_rel >= 0.0) || !std::isfinite(tol_rel)) return INVALID;
    if (!(border >= 0.0) || !std::isfinite(border)) return INVALID;
    if (n == 0) return EMPTY;
    if (!points || !cameras || !depths) return INVALID;
    if (!seen || !agree || !violate || !residual) return INVALID;
    return LAUNCH;
}

// ---- what the kernel finds its point and addresses the arrays with (constexpr: the same
// functions on the device) ----
// (one thread per point and no grid-stride loop: every point needs its block, however many)
constexpr int64_t blocks(int64_t n, int block) { return (n + block - 1) / block; }
constexpr bool point_in(int64_t i, int64_t n) { return i >= 0 && i < n; }
// coordinate k of point i of a [3][n] table: three streams, each contiguous over the points
constexpr size_t coord_index(int k, int64_t i, int64_t n) {
    return (size_t)k * (size_t)n + (size_t)i;
}
// floats of a [V][H][W] map
constexpr size_t map_extent(int V, int H, int W) {
    return V > 0 ? map_index(V - 1, H - 1, W - 1, H, W) + 1 : 0;
}

// ---- what one view says about one point.  in_view: rn_view::project's ok; zm: the depth the
// view recorded at the point's pixel; dd: the squared distance of the point from the view's
// centre.  A view measures where it is in view and 0 < zm < inf; a measuring view agrees where
// -t <= s <= t, is violated where s > t (it sees past the point: the point floats in its free
// space) and is merely occluded where s < -t.  Every test is a comparison that a NaN fails. ----
struct Vote {
    bool measured, agrees, violates;
    double s;
};
__attribute__((always_inline)) constexpr Vote classify(bool in_view, double zm, double dd,
                                                       double tol_abs, double tol_rel) {
    const bool measured = in_view && zm > 0.0 && zm < INFINITY;
    const double s = (zm * zm - dd) / (zm + zm);
    const double t = tol_abs + tol_rel * zm;
    return Vote{measured, measured && s >= -t && s <= t, measured && s > t, s};
}

}  // namespace rn_consistency
