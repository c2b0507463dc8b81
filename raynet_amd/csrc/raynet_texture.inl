// raynet_texture.inl -- the photographs baked into a texture atlas of a surface mesh, and the
// lookup behind a render (the definitions are in include/raynet_hip.h at
// rn_texture_bake / rn_texture_sample).  Included at the end of raynet_hip.hip, behind
// raynet_render.inl.
//
//   k_texture_bake<C, TILED>  one lane per texel of the atlas.  The texel's owner and its place in
//                             the chart are integer arithmetic (raynet_texture_args.h); its point
//                             on the face and the normal there are formed in fp64 and stay fp64;
//                             then, for the views in ascending order, rn_project_colors's
//                             per-view step, called (rn_view::observe of raynet_views_args.h):
//                             projection, the in-view, facing and occlusion tests, a bilinear
//                             fetch of C channels, the blend or the best view.  The camera rows
//                             are the same for every lane (scalar loads); nothing is shared
//                             between lanes.
//   k_texture_sample<C>       one lane per pixel of rn_mesh_render's face / bary planes: the chart
//                             position of (u, v), a bilinear or nearest fetch from the atlas.
//
// TILED: a wavefront covers an 8 x 8 tile of texels -- neighbouring texels of a chart fetch
// neighbouring pixels; else 64 texels of a row, which span three or more charts.  The result does
// not depend on the mapping; TEXTURE_TILED, one constant, chooses it when the library is built.
//
// Plain HIP C++.  Every fp64 operation of the definitions is rounded on its own and in the stated
// order (-ffp-contract=off; the divisions are IEEE; no square root anywhere):
// tests/texture_truth.py restates them in np.float64 and the GPU tests ask for the same bits.

#include "raynet_texture_args.h"

namespace {

constexpr bool TEXTURE_TILED = true;    // (tools/texture_bench.py --build_rows builds the other one)

struct BakeArgs {
    int64_t nv, nf;
    const float *vertices;
    const int32_t *faces;
    const float *normals;                   // null: the face's e1 x e2
    int32_t T, Cw;
    int64_t Wt, Ht;
    int V;
    const double *cameras;
    int H, W;
    const float *images, *depths;           // depths: null for none
    double tol, min_cos, border;
    int mode;
    float *texture, *weight;
    uint32_t *views;
};

// a = (Wb a0 + u a1) + v a2 in fp64
__device__ __forceinline__ double texture_mix(double Wb, double u, double v, double a0, double a1,
                                              double a2) {
    return (Wb * a0 + u * a1) + v * a2;
}

template <int C, bool TILED>
__global__ __launch_bounds__(BLOCK) void k_texture_bake(BakeArgs a) {
    static_assert(BLOCK % rn_tex::TILE_TEXELS == 0 && rn_tex::TILE_TEXELS == WAVE,
                  "a tile is a wavefront");
    const int64_t lane = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    const rn_tex::Texel tx =
        TILED ? rn_tex::texel_of_tile(lane / rn_tex::TILE_TEXELS,
                                      (int)(lane % rn_tex::TILE_TEXELS), a.Wt, a.Ht)
              : rn_tex::texel_of_row(lane, a.Wt, a.Ht);
    if (tx.x < 0) return;
    const size_t at = rn_tex::texel_index(tx.x, tx.y, a.Wt);
    const rn_tex::Owner o = rn_tex::owner_of(tx.x, tx.y, a.nf, a.T, a.Cw);
    int32_t i0 = -1, i1 = -1, i2 = -1;
    if (rn_tex::face_in(o.face, a.nf)) {
        i0 = a.faces[rn_tex::xyz_index(o.face, 0)];
        i1 = a.faces[rn_tex::xyz_index(o.face, 1)];
        i2 = a.faces[rn_tex::xyz_index(o.face, 2)];
    }
    const bool known = rn_tex::face_in(o.face, a.nf) && rn_tex::vertex_in(i0, a.nv) &&
                       rn_tex::vertex_in(i1, a.nv) && rn_tex::vertex_in(i2, a.nv);
    if (!known) {       // an empty texel, or a face that names no three vertices
#pragma unroll
        for (int c = 0; c < C; c++) a.texture[at * C + c] = 0.0f;
        a.weight[at] = 0.0f;
        a.views[at] = 0u;
        return;
    }
    // onto the triangle: a gutter texel takes a point of its face's rim
    const double u0 = rn_tex::raw_coordinate(o.lower, o.i, a.T),
                 v0 = rn_tex::raw_coordinate(o.lower, o.j, a.T);
    double u = u0 > 0.0 ? u0 : 0.0, v = v0 > 0.0 ? v0 : 0.0;
    const double s = u + v;
    if (s > 1.0) {
        u = u / s;
        v = v / s;
    }
    const double Wb = (1.0 - u) - v;
    double p0[3], p1[3], p2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p0[k] = (double)a.vertices[rn_tex::xyz_index(i0, k)];
        p1[k] = (double)a.vertices[rn_tex::xyz_index(i1, k)];
        p2[k] = (double)a.vertices[rn_tex::xyz_index(i2, k)];
    }
    const double x = texture_mix(Wb, u, v, p0[0], p1[0], p2[0]),
                 y = texture_mix(Wb, u, v, p0[1], p1[1], p2[1]),
                 z = texture_mix(Wb, u, v, p0[2], p1[2], p2[2]);
    double nx, ny, nz;
    if (a.normals) {
        nx = texture_mix(Wb, u, v, (double)a.normals[rn_tex::xyz_index(i0, 0)],
                         (double)a.normals[rn_tex::xyz_index(i1, 0)],
                         (double)a.normals[rn_tex::xyz_index(i2, 0)]);
        ny = texture_mix(Wb, u, v, (double)a.normals[rn_tex::xyz_index(i0, 1)],
                         (double)a.normals[rn_tex::xyz_index(i1, 1)],
                         (double)a.normals[rn_tex::xyz_index(i2, 1)]);
        nz = texture_mix(Wb, u, v, (double)a.normals[rn_tex::xyz_index(i0, 2)],
                         (double)a.normals[rn_tex::xyz_index(i1, 2)],
                         (double)a.normals[rn_tex::xyz_index(i2, 2)]);
    } else {
        const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
        const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
        nx = e1y * e2z - e1z * e2y;
        ny = e1z * e2x - e1x * e2z;
        nz = e1x * e2y - e1y * e2x;
    }
    // rn_project_colors's per-view step, on the fp64 point and normal
    const rn_view::Views views{a.V, a.cameras, a.H, a.W, a.images, a.depths, a.tol, a.min_cos,
                               a.border, a.mode};
    const rn_view::Observation<C> seen = rn_view::observe<C>(views, x, y, z, nx, ny, nz);
#pragma unroll
    for (int c = 0; c < C; c++) a.texture[at * C + c] = seen.color[c];
    a.weight[at] = seen.weight;
    a.views[at] = seen.views;
}

struct SampleArgs {
    int64_t n;
    const int32_t *face;
    const float *bary;
    int64_t nf;
    int32_t T, Cw;
    int64_t Wt, Ht;
    const float *texture;
    int bilinear;
    float *color;
};

template <int C>
__global__ __launch_bounds__(BLOCK) void k_texture_sample(SampleArgs a) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const int64_t f = a.face[i];
    const double U = (double)a.bary[2 * i], Vb = (double)a.bary[2 * i + 1];
    // a NaN fails every comparison
    const bool known = rn_tex::face_in(f, a.nf) && U >= 0.0 && U <= 1.0 && Vb >= 0.0 && Vb <= 1.0;
    float out[C];
#pragma unroll
    for (int c = 0; c < C; c++) out[c] = 0.0f;
    if (known) {
        const int32_t S = a.T + rn_tex::MARGIN;
        const bool lower = rn_tex::is_lower(f);
        // within [1, T + 3] of the cell: the whole footprint lies inside the cell
        const double x = (double)(rn_tex::cell_column(f, a.Cw) * S) +
                         rn_tex::chart_coordinate(lower, U, a.T),
                     y = (double)(rn_tex::cell_row(f, a.Cw) * S) +
                         rn_tex::chart_coordinate(lower, Vb, a.T);
        if (a.bilinear) {
            const double xf = floor(x), yf = floor(y);
            const double fx = x - xf, fy = y - yf;
            const int64_t x0 = (int64_t)xf, y0 = (int64_t)yf;
            const int64_t x1 = min(x0 + 1, a.Wt - 1), y1 = min(y0 + 1, a.Ht - 1);
#pragma unroll
            for (int c = 0; c < C; c++) {
                const double t00 = a.texture[rn_tex::texel_index(x0, y0, a.Wt) * C + c],
                             t01 = a.texture[rn_tex::texel_index(x1, y0, a.Wt) * C + c],
                             t10 = a.texture[rn_tex::texel_index(x0, y1, a.Wt) * C + c],
                             t11 = a.texture[rn_tex::texel_index(x1, y1, a.Wt) * C + c];
                out[c] = (float)rn_view::bilerp(t00, t01, t10, t11, fx, fy);
            }
        } else {
            const int64_t xr = (int64_t)rint(x), yr = (int64_t)rint(y);     // half to even
#pragma unroll
            for (int c = 0; c < C; c++) out[c] = a.texture[rn_tex::texel_index(xr, yr, a.Wt) * C + c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) a.color[(size_t)i * C + c] = out[c];
}

}  // namespace

extern "C" {

int rn_texture_bake(rn_ctx *ctx, int64_t nv, const float *vertices, int64_t nf, const int32_t *faces,
                    const float *normals, int32_t T, int32_t cells_per_row, int32_t V,
                    const double *cameras, int32_t H, int32_t W, int32_t C, const float *images,
                    const float *depths, double tol, double min_cos, double border, int32_t mode,
                    float *texture, float *weight, uint32_t *views, void *stream) {
    const rn_tex::Verdict verdict =
        rn_tex::bake_args(ctx != nullptr, nv, vertices, nf, faces, T, cells_per_row, V, cameras, H,
                          W, C, images, tol, min_cos, border, mode, texture, weight, views);
    if (verdict == rn_tex::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_texture_bake: bad argument (nv %lld, nf %lld, T %d, "
                    "cells_per_row %d, V %d, H %d, W %d, C %d, tol %g, min_cos %g, border %g, "
                    "mode %d)", (long long)nv, (long long)nf, (int)T, (int)cells_per_row, (int)V,
                    (int)H, (int)W, (int)C, tol, min_cos, border, (int)mode);
    if (verdict == rn_tex::EMPTY) return RN_OK;
    const rn_tex::Layout L = rn_tex::layout_of(nf, T, cells_per_row);
    const BakeArgs a{nv, nf, vertices, faces, normals, T, cells_per_row, L.Wt, L.Ht, V, cameras, H,
                     W, images, depths, tol, min_cos, border, mode, texture, weight, views};
    const int64_t lanes = TEXTURE_TILED ? rn_tex::lanes_tiled(L.Wt, L.Ht)
                                        : rn_tex::lanes_rows(L.Wt, L.Ht);
    const dim3 grid((unsigned)rn_tex::blocks(lanes, BLOCK));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, S(stream), a);
    };
    if (C == 1) go(k_texture_bake<1, TEXTURE_TILED>);
    else if (C == 2) go(k_texture_bake<2, TEXTURE_TILED>);
    else if (C == 3) go(k_texture_bake<3, TEXTURE_TILED>);
    else go(k_texture_bake<4, TEXTURE_TILED>);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_texture_sample(rn_ctx *ctx, int64_t n, const int32_t *face, const float *bary, int64_t nf,
                      int32_t T, int32_t cells_per_row, int32_t C, const float *texture,
                      int32_t bilinear, float *color, void *stream) {
    const rn_tex::Verdict verdict = rn_tex::sample_args(ctx != nullptr, n, face, bary, nf, T,
                                                        cells_per_row, C, texture, bilinear, color);
    if (verdict == rn_tex::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_texture_sample: bad argument (n %lld, nf %lld, T %d, "
                    "cells_per_row %d, C %d, bilinear %d)", (long long)n, (long long)nf, (int)T,
                    (int)cells_per_row, (int)C, (int)bilinear);
    if (verdict == rn_tex::EMPTY) return RN_OK;
    const rn_tex::Layout L = rn_tex::layout_of(nf, T, cells_per_row);
    const SampleArgs a{n, face, bary, nf, T, cells_per_row, L.Wt, L.Ht, texture, bilinear, color};
    const dim3 grid((unsigned)rn_tex::blocks(n, BLOCK));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, S(stream), a);
    };
    if (C == 1) go(k_texture_sample<1>);
    else if (C == 2) go(k_texture_sample<2>);
    else if (C == 3) go(k_texture_sample<3>);
    else go(k_texture_sample<4>);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
