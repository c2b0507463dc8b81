// raynet_fusion_args.h -- the argument checks and the index arithmetic of rn_tsdf_integrate
// (raynet_fusion.inl), host-only and free of HIP so that they compile into a stand-alone program
// (tests/fusion_args_main.cpp, built with the address and undefined-behaviour sanitizers by
// tests/test_fusion_cpu.py).  The launcher acts on the verdict; the kernel finds its voxel and
// addresses the maps with the constexpr functions below.
//
// The signed distance of the definition, s = (z z - dd) / (z + z), is (z - r)(z + r) / 2z with
// r = sqrt(dd): zero exactly where r = z, monotone in r, within the band off z - r by the factor
// 1 - (z - r) / 2z -- and free of a square root, so that a NumPy restatement gives the same bits
// (tests/fusion_truth.py).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_views_args.h"

namespace rn_fusion {

// the camera rows, and pixel (view, y, x) of a [V][H][W] map: a pixel coordinate of a view that
// counts lies in [0, extent - 1]; everything else reads pixel 0
using rn_view::CAMERA_DOUBLES, rn_view::map_index, rn_view::pixel_in;

constexpr int MAX_VIEWS = 4096;         // rejects garbage; not a capacity

enum Verdict { INVALID = -1, LAUNCH = 1 };

// rn_tsdf_integrate.  Never empty: a context rn_create admitted has G >= 1 voxels, and all of
// them are written also with V == 0.  cameras and depths are read only where there are views;
// weights may be null (weight 1).
inline Verdict integrate_args(bool have_ctx, int32_t V, const void *cameras, int32_t H, int32_t W,
                              const void *depths, double trunc, double border, const void *tsdf,
                              const void *weight) {
    if (!have_ctx) return INVALID;
    if (V < 0 || V > MAX_VIEWS) return INVALID;
    if (H < 1 || W < 1) return INVALID;
    if (!(trunc > 0.0) || !std::isfinite(trunc)) return INVALID;
    if (!(border >= 0.0) || !std::isfinite(border)) return INVALID;
    if (!tsdf || !weight) return INVALID;
    if (V > 0 && (!cameras || !depths)) return INVALID;
    return LAUNCH;
}

// ---- what the kernel finds its voxel and addresses the maps with (constexpr: the same functions
// on the device) ----
constexpr int64_t voxels(int32_t gx, int32_t gy, int32_t gz) {
    return (int64_t)gx * (int64_t)gy * (int64_t)gz;
}
// (one thread per voxel and no grid-stride loop: every voxel needs its block, however many)
constexpr int64_t blocks(int64_t G, int block) { return (G + block - 1) / block; }
constexpr bool voxel_in(int64_t g, int64_t G) { return g >= 0 && g < G; }

// voxel g of a [gx][gy][gz] grid (z fastest) -> (i, j, k)
struct Voxel {
    int32_t i, j, k;
};
constexpr Voxel voxel_of(int64_t g, int32_t gy, int32_t gz) {
    return Voxel{(int32_t)(g / gz / gy), (int32_t)(g / gz % gy), (int32_t)(g % gz)};
}
constexpr int64_t voxel_index(int32_t i, int32_t j, int32_t k, int32_t gy, int32_t gz) {
    return ((int64_t)i * gy + j) * gz + k;
}
// the entries of the context's axis table (x | y | z) that hold a voxel's centre
constexpr int axis_x(const Voxel &v) { return v.i; }
constexpr int axis_y(const Voxel &v, int32_t gx) { return gx + v.j; }
constexpr int axis_z(const Voxel &v, int32_t gx, int32_t gy) { return gx + gy + v.k; }

// floats of a [V][H][W] map
constexpr size_t map_extent(int V, int H, int W) {
    return V > 0 ? map_index(V - 1, H - 1, W - 1, H, W) + 1 : 0;
}

}  // namespace rn_fusion
