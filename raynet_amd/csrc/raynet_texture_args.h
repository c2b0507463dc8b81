// raynet_texture_args.h -- the atlas layout, the argument checks and the index arithmetic of
// rn_texture_bake / rn_texture_sample (raynet_texture.inl), host-only and free of HIP so that they
// compile into a stand-alone program (tests/texture_args_main.cpp, built with the address and
// undefined-behaviour sanitizers by tests/test_texture_cpu.py).  The launchers act on the
// verdicts; the kernels find their texel with texel_of_tile / texel_of_row, its owner with
// owner_of and a chart position with chart_coordinate.  The limits of a mesh's sizes and the guards
// of its indices are raynet_mesh_args.h's, the per-view scalars raynet_appearance_args.h's.  The
// functions are constexpr only so that the device may call them.
//
// The definitions are in include/raynet_hip.h at rn_texture_bake.
#pragma once

#include <cstddef>
#include <cstdint>

#include "raynet_appearance_args.h"
#include "raynet_mesh_args.h"

namespace rn_tex {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::sizes_ok, rn_mesh::vertex_in, rn_mesh::face_in;
using rn_mesh::xyz_index;

constexpr int MIN_T = 1, MAX_T = 1024;      // texel steps along a chart's leg
constexpr int MARGIN = 5;                   // a cell is T + MARGIN texels square
constexpr int MAX_CELLS_PER_ROW = 16384;    // rejects garbage; the extent is what binds
constexpr int MAX_EXTENT = 16384;           // texels along either side of the atlas
constexpr int MIN_CHANNELS = 1, MAX_CHANNELS = rn_app::MAX_CHANNELS;
constexpr int TILE = 8;                     // a wavefront covers TILE x TILE texels
constexpr int TILE_TEXELS = TILE * TILE;

// ---- the layout: two faces per cell of S x S texels, Cw cells per row ----
struct Layout {
    int32_t T, S, Cw;
    int64_t cells, rows, Wt, Ht;            // Wt = Cw S whatever nf; Ht = rows S (0 without faces)
};
constexpr bool steps_ok(int32_t T) { return T >= MIN_T && T <= MAX_T; }
constexpr bool cells_per_row_ok(int32_t Cw) { return Cw >= 1 && Cw <= MAX_CELLS_PER_ROW; }
// (nf <= INT32_LIMIT / 3, T and Cw in range: nothing here overflows an int64)
constexpr Layout layout_of(int64_t nf, int32_t T, int32_t Cw) {
    const int64_t cells = (nf + 1) / 2, rows = (cells + Cw - 1) / Cw;
    const int32_t S = T + MARGIN;
    return Layout{T, S, Cw, cells, rows, (int64_t)Cw * S, rows * S};
}
// the atlas is small enough to be addressed: both extents, and an entry of `texture` as an int32
constexpr bool extents_ok(const Layout &L) {
    return L.cells == 0 || (L.Wt <= MAX_EXTENT && L.Ht <= MAX_EXTENT);
}

// ---- who owns texel (tx, ty) of the atlas ----
struct Owner {
    int64_t face;       // -1: nobody (the upper half of an odd nf's last cell, the trailing cells)
    int32_t i, j;       // the texel within its cell
    bool lower;
};
constexpr Owner owner_of(int64_t tx, int64_t ty, int64_t nf, int32_t T, int32_t Cw) {
    const int32_t S = T + MARGIN;
    const int64_t cx = tx / S, cy = ty / S;
    const int32_t i = (int32_t)(tx % S), j = (int32_t)(ty % S);
    const bool lower = i + j <= T + 3;
    const int64_t f = 2 * (cy * Cw + cx) + (lower ? 0 : 1);
    return Owner{face_in(f, nf) ? f : -1, i, j, lower};
}
// the cell of face f: (column, row)
constexpr int64_t cell_column(int64_t f, int32_t Cw) { return f / 2 % Cw; }
constexpr int64_t cell_row(int64_t f, int32_t Cw) { return f / 2 / Cw; }
constexpr bool is_lower(int64_t f) { return f % 2 == 0; }

// A texel's raw barycentric along one axis (i for u, j for v): the inverse of chart_coordinate at
// whole positions, negative or beyond 1 in the gutter.
constexpr double raw_coordinate(bool lower, int32_t at, int32_t T) {
    return lower ? (double)(at - 1) / (double)T : (double)((T + 3) - at) / (double)T;
}
// Where the barycentric u (or v) lies along its axis of the chart, in cell-local texels.
constexpr double chart_coordinate(bool lower, double u, int32_t T) {
    return lower ? 1.0 + u * (double)T : (double)(T + 3) - u * (double)T;
}

// ---- where a lane's texel is.  Both mappings name every texel of the atlas exactly once, and
// lanes beyond them none ----
struct Texel {
    int64_t x, y;       // x < 0: the lane has no texel
};
constexpr int64_t tiles_across(int64_t extent) { return (extent + TILE - 1) / TILE; }
constexpr Texel texel_of_tile(int64_t tile, int lane, int64_t Wt, int64_t Ht) {
    const int64_t across = tiles_across(Wt);
    if (tile < 0 || across < 1 || tile / across >= tiles_across(Ht)) return Texel{-1, 0};
    const int64_t y = tile / across * TILE + lane / TILE, x = tile % across * TILE + lane % TILE;
    if (x >= Wt || y >= Ht) return Texel{-1, 0};
    return Texel{x, y};
}
constexpr Texel texel_of_row(int64_t i, int64_t Wt, int64_t Ht) {
    if (i < 0 || Wt < 1 || i / Wt >= Ht) return Texel{-1, 0};
    return Texel{i % Wt, i / Wt};
}
constexpr int64_t lanes_tiled(int64_t Wt, int64_t Ht) {
    return tiles_across(Wt) * tiles_across(Ht) * TILE_TEXELS;
}
constexpr int64_t lanes_rows(int64_t Wt, int64_t Ht) { return Wt * Ht; }
constexpr int64_t blocks(int64_t lanes, int block) { return (lanes + block - 1) / block; }
// texel (x, y) of a [Ht][Wt] plane
constexpr size_t texel_index(int64_t x, int64_t y, int64_t Wt) {
    return (size_t)y * (size_t)Wt + (size_t)x;
}

// rn_texture_bake.  The mesh's sizes and the layout first, then everything rn_project_colors
// refuses about its scalars, with the atlas's texels as its points (which also bounds Wt Ht C),
// no face: EMPTY whatever the pointers; then the pointers.
inline Verdict bake_args(bool have_ctx, int64_t nv, const void *vertices, int64_t nf,
                         const void *faces, int32_t T, int32_t Cw, int32_t V, const void *cameras,
                         int32_t H, int32_t W, int32_t C, const void *images, double tol,
                         double min_cos, double border, int32_t mode, const void *texture,
                         const void *weight, const void *views) {
    if (!have_ctx || !sizes_ok(nv, nf)) return INVALID;
    if (!steps_ok(T) || !cells_per_row_ok(Cw)) return INVALID;
    const Layout L = layout_of(nf, T, Cw);
    if (!extents_ok(L)) return INVALID;
    const Verdict v = rn_app::colors_args(true, L.Wt * L.Ht, vertices, V, cameras, H, W, C, images,
                                          tol, min_cos, border, mode, texture, weight, views);
    if (v != LAUNCH) return v;
    if (!faces) return INVALID;
    return LAUNCH;
}

// rn_texture_sample, in the same order: the scalars, no pixel: EMPTY, the pointers.  Without faces
// every pixel is a miss and the atlas is never read.
inline Verdict sample_args(bool have_ctx, int64_t n, const void *face, const void *bary, int64_t nf,
                           int32_t T, int32_t Cw, int32_t C, const void *texture, int32_t bilinear,
                           const void *color) {
    if (!have_ctx || n < 0 || !sizes_ok(0, nf)) return INVALID;
    if (!steps_ok(T) || !cells_per_row_ok(Cw)) return INVALID;
    if (C < MIN_CHANNELS || C > MAX_CHANNELS) return INVALID;
    if (bilinear != 0 && bilinear != 1) return INVALID;
    if (n > INT32_LIMIT / C) return INVALID;        // an entry n C + c of `color` is an int32
    const Layout L = layout_of(nf, T, Cw);
    if (!extents_ok(L) || L.Wt * L.Ht > INT32_LIMIT / C) return INVALID;
    if (n == 0) return EMPTY;
    if (!face || !bary || !color) return INVALID;
    if (nf > 0 && !texture) return INVALID;
    return LAUNCH;
}

}  // namespace rn_tex
