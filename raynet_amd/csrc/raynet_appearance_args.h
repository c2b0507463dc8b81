// raynet_appearance_args.h -- the argument checks and the index arithmetic of
// rn_vertex_area_normals / rn_project_colors (raynet_appearance.inl), host-only and free of HIP so
// that they compile into a stand-alone program (tests/appearance_args_main.cpp, built with the
// address and undefined-behaviour sanitizers by tests/test_appearance_cpu.py).  The launchers act
// on the verdicts; the kernels guard and address their reads with the mesh guards of
// raynet_mesh_args.h, and k_project_colors's per-view step is raynet_views_args.h's observe.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_mesh_args.h"
#include "raynet_views_args.h"

namespace rn_app {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::sizes_ok;
using rn_mesh::vertex_in, rn_mesh::corner_in, rn_mesh::clamp_slot, rn_mesh::xyz_index;
using rn_view::CAMERA_DOUBLES, rn_view::image_index, rn_view::pixel_in;

constexpr int MAX_VIEWS = 32;           // one bit of the `views` word each
constexpr int MAX_CHANNELS = 4;

// rn_vertex_area_normals.  The scalars first, then nv == 0 (nothing to write: EMPTY, whatever the
// pointers), then the pointers: faces and corners are read only where there are faces.
inline Verdict normals_args(bool have_ctx, int64_t nv, const void *vertices, int64_t nf,
                            const void *faces, const void *offsets, const void *corners,
                            const void *normals) {
    if (!have_ctx || !sizes_ok(nv, nf)) return INVALID;
    if (nv == 0) return EMPTY;
    if (!vertices || !offsets || !normals) return INVALID;
    if (nf > 0 && (!faces || !corners)) return INVALID;
    return LAUNCH;
}

// rn_project_colors, in the same order.  images and cameras are read only where there are views;
// normals and depths may be null (no facing test / no occlusion test).
inline Verdict colors_args(bool have_ctx, int64_t n, const void *points, int32_t V,
                           const void *cameras, int32_t H, int32_t W, int32_t C,
                           const void *images, double tol, double min_cos, double border,
                           int32_t mode, const void *colors, const void *weight,
                           const void *views) {
    if (!have_ctx || n < 0) return INVALID;
    if (V < 0 || V > MAX_VIEWS) return INVALID;
    if (C < 1 || C > MAX_CHANNELS) return INVALID;
    if (H < 1 || W < 1) return INVALID;
    if (n > INT32_LIMIT / C) return INVALID;        // an entry n C + c of `colors` is an int32
    if (!(tol >= 0.0) || !std::isfinite(tol)) return INVALID;
    if (!(min_cos >= 0.0) || !(min_cos < 1.0)) return INVALID;
    if (!(border >= 0.0) || !std::isfinite(border)) return INVALID;
    if (mode != 0 && mode != 1) return INVALID;
    if (n == 0) return EMPTY;
    if (!points || !colors || !weight || !views) return INVALID;
    if (V > 0 && (!cameras || !images)) return INVALID;
    return LAUNCH;
}

// ---- what the kernels guard and address with (constexpr: the same functions on the device):
// rn_mesh's for the mesh, rn_view's for the images.  depth_index: pixel (view, y, x) of a
// [V][H][W] map ----
constexpr size_t depth_index(int v, int y, int x, int H, int W) {
    return rn_view::map_index(v, y, x, H, W);
}

}  // namespace rn_app
