// raynet_render_args.h -- the argument checks and the index arithmetic of rn_mesh_render
// (raynet_render.inl), host-only and free of HIP so that they compile into a stand-alone program
// (tests/render_args_main.cpp, built with the address and undefined-behaviour sanitizers by
// tests/test_render_cpu.py).  The launcher acts on the verdict; the kernel finds its pixel with
// pixel_of_tile / pixel_of_row and addresses the outputs with pixel_index.  The limits of a mesh's
// sizes and the guards of its indices are raynet_mesh_args.h's.  The functions are constexpr only
// so that the device may call them.
//
// The definition is in include/raynet_hip.h at rn_mesh_render.
#pragma once

#include <cstddef>
#include <cstdint>

#include "raynet_mesh_args.h"

namespace rn_render {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::sizes_ok, rn_mesh::vertex_in, rn_mesh::face_in;
using rn_mesh::xyz_index;

constexpr int MAX_VIEWS = 4096;         // rejects garbage; not a capacity
constexpr int CAMERA_FLOATS = 15;       // P_pinv [4][3] row-major | centre [3]
constexpr int MIN_CHANNELS = 1, MAX_CHANNELS = 4;
constexpr int TILE = 8;                 // a wavefront covers TILE x TILE pixels
constexpr int TILE_PIXELS = TILE * TILE;

// V * H * W, or -1 where it does not fit the int32 the outputs are counted with.  No view: no
// pixel, whatever H and W (both >= 0, V in [0, MAX_VIEWS]: nothing here overflows an int64).
constexpr int64_t pixels(int64_t V, int64_t H, int64_t W) {
    if (V == 0 || H == 0 || W == 0) return 0;
    if (H > INT32_LIMIT / W) return -1;
    return V * (H * W) > INT32_LIMIT ? -1 : V * (H * W);
}

// rn_mesh_render.  The scalars first (C counts only where there are colours), then nothing to do
// (no view or no pixel: EMPTY, whatever the pointers), then the pointers: the required ones, and
// that an attribute and its image come together.
inline Verdict render_args(bool have_ctx, const void *nodes, const void *leaves, int64_t nv,
                           const void *vertices, int64_t nf, const void *faces, const void *colors,
                           int32_t C, const void *normals, int32_t V, const void *cameras,
                           int32_t H, int32_t W, const void *face, const void *depth,
                           const void *bary, const void *color, const void *normal) {
    if (!have_ctx) return INVALID;
    if (V < 0 || H < 0 || W < 0 || V > MAX_VIEWS) return INVALID;
    if (!sizes_ok(nv, nf) || nf < 1) return INVALID;
    const int64_t n = pixels(V, H, W);
    if (n < 0) return INVALID;
    if (colors && (C < MIN_CHANNELS || C > MAX_CHANNELS || n * C > INT32_LIMIT)) return INVALID;
    if (n == 0) return EMPTY;
    if (!nodes || !leaves || !vertices || !faces || !cameras) return INVALID;
    if (!face || !depth || !bary) return INVALID;
    if ((colors == nullptr) != (color == nullptr)) return INVALID;
    if ((normals == nullptr) != (normal == nullptr)) return INVALID;
    return LAUNCH;
}

// ---- where a lane's pixel is.  Both mappings name every pixel of every view exactly once, and
// lanes beyond them none ----
struct Pixel {
    int32_t view, row, column;      // view < 0: the lane has no pixel
};
constexpr int64_t tiles_across(int32_t W) { return ((int64_t)W + TILE - 1) / TILE; }
constexpr int64_t tiles_of_view(int32_t H, int32_t W) { return tiles_across(H) * tiles_across(W); }
// lane `lane` in [0, TILE_PIXELS) of tile `tile`; the tiles of a view row by row, the views one
// after the other; a tile that hangs over the image's right or lower edge has idle lanes
constexpr Pixel pixel_of_tile(int64_t tile, int lane, int32_t V, int32_t H, int32_t W) {
    const int64_t per_view = tiles_of_view(H, W);
    if (tile < 0 || per_view < 1 || tile / per_view >= V) return Pixel{-1, 0, 0};
    const int64_t t = tile % per_view;
    const int64_t row = t / tiles_across(W) * TILE + lane / TILE;
    const int64_t column = t % tiles_across(W) * TILE + lane % TILE;
    if (row >= H || column >= W) return Pixel{-1, 0, 0};
    return Pixel{(int32_t)(tile / per_view), (int32_t)row, (int32_t)column};
}
// item i of [0, V H W): the pixels of a view row by row
constexpr Pixel pixel_of_row(int64_t i, int32_t V, int32_t H, int32_t W) {
    const int64_t per_view = (int64_t)H * W;
    if (i < 0 || per_view < 1 || i / per_view >= V) return Pixel{-1, 0, 0};
    return Pixel{(int32_t)(i / per_view), (int32_t)(i % per_view / W), (int32_t)(i % per_view % W)};
}
// how many lanes each mapping needs, and the workgroups of `block` lanes that hold them
constexpr int64_t lanes_tiled(int32_t V, int32_t H, int32_t W) {
    return (int64_t)V * tiles_of_view(H, W) * TILE_PIXELS;
}
constexpr int64_t lanes_rows(int32_t V, int32_t H, int32_t W) { return (int64_t)V * H * W; }
constexpr int64_t blocks(int64_t lanes, int block) { return (lanes + block - 1) / block; }

// pixel (view, row, column) of a [V][H][W] image
constexpr size_t pixel_index(const Pixel &p, int32_t H, int32_t W) {
    return ((size_t)p.view * (size_t)H + (size_t)p.row) * (size_t)W + (size_t)p.column;
}

}  // namespace rn_render
