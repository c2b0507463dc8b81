// raynet_appearance.inl -- what a surface looks like: area-weighted vertex normals of an indexed
// mesh and the colours the scene's images give to points (the definitions
// are in include/raynet_hip.h at rn_vertex_area_normals / rn_project_colors).  Included at the end
// of raynet_hip.hip.
//
//   k_vertex_area_normals  one thread per vertex: the sum of e1 x e2 over the faces around it, in
//                          the order of its row of the corner table (a CSR by vertex), in fp64.
//   k_project_colors<C>    one thread per point, the views in ascending order: projection, the
//                          in-view, facing and occlusion tests, a bilinear fetch of C channels,
//                          the blend or the best view.  The camera rows are the same for every
//                          lane (scalar loads); no LDS, no atomics, nothing shared between threads.
//
// Plain HIP C++.  Every fp64 operation of the definitions is rounded on its own and in the stated
// order (-ffp-contract=off; the divisions are IEEE; no sqrt anywhere): tests/appearance_truth.py
// restates them in np.float64 and the GPU tests ask for the same bits.

#include "raynet_appearance_args.h"

namespace {

__global__ __launch_bounds__(BLOCK) void k_vertex_area_normals(
        int64_t nv, const float *__restrict__ vertices, int64_t nf,
        const int32_t *__restrict__ faces, const int32_t *__restrict__ offsets,
        const int32_t *__restrict__ corners, float *normals) {
    const int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (!rn_app::vertex_in(v, nv)) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    // (offsets may hold anything: the range is cut to the entries `corners` has; nf == 0: empty)
    const int64_t first = rn_app::clamp_slot(offsets[v], nf),
                  last = rn_app::clamp_slot(offsets[v + 1], nf);
    for (int64_t k = first; k < last; k++) {
        const int64_t c = corners[k];
        if (!rn_app::corner_in(c, nf)) continue;
        const int64_t f = c / 3;
        const int64_t i0 = faces[rn_app::xyz_index(f, 0)], i1 = faces[rn_app::xyz_index(f, 1)],
                      i2 = faces[rn_app::xyz_index(f, 2)];
        if (!rn_app::vertex_in(i0, nv) || !rn_app::vertex_in(i1, nv) || !rn_app::vertex_in(i2, nv))
            continue;
        const double p0x = vertices[rn_app::xyz_index(i0, 0)],
                     p0y = vertices[rn_app::xyz_index(i0, 1)],
                     p0z = vertices[rn_app::xyz_index(i0, 2)];
        const double e1x = (double)vertices[rn_app::xyz_index(i1, 0)] - p0x,
                     e1y = (double)vertices[rn_app::xyz_index(i1, 1)] - p0y,
                     e1z = (double)vertices[rn_app::xyz_index(i1, 2)] - p0z;
        const double e2x = (double)vertices[rn_app::xyz_index(i2, 0)] - p0x,
                     e2y = (double)vertices[rn_app::xyz_index(i2, 1)] - p0y,
                     e2z = (double)vertices[rn_app::xyz_index(i2, 2)] - p0z;
        sx = sx + (e1y * e2z - e1z * e2y);
        sy = sy + (e1z * e2x - e1x * e2z);
        sz = sz + (e1x * e2y - e1y * e2x);
    }
    normals[rn_app::xyz_index(v, 0)] = (float)sx;
    normals[rn_app::xyz_index(v, 1)] = (float)sy;
    normals[rn_app::xyz_index(v, 2)] = (float)sz;
}

struct ColorArgs {
    int64_t n;
    const float *points, *normals;          // normals: null for none
    int V;
    const double *cameras;
    int H, W;
    const float *images, *depths;           // depths: null for none
    double tol, min_cos, border;
    int mode;
    float *colors, *weight;
    uint32_t *views;
};

template <int C>
__global__ __launch_bounds__(BLOCK) void k_project_colors(ColorArgs a) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const double x = a.points[rn_app::xyz_index(i, 0)], y = a.points[rn_app::xyz_index(i, 1)],
                 z = a.points[rn_app::xyz_index(i, 2)];
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (a.normals) {
        nx = a.normals[rn_app::xyz_index(i, 0)];
        ny = a.normals[rn_app::xyz_index(i, 1)];
        nz = a.normals[rn_app::xyz_index(i, 2)];
    }
    // rn_view::observe<C> (raynet_views_args.h), written out: through the call this kernel's code
    // changes and two of seven timed figures were slower than this text's by more than the
    // noise (profiles/view_step_bench.json).  The bake of an atlas calls it, and a GPU test
    // holds the two to the same bits at the corners of the charts.
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const bool facing = nn > 0.0;                       // (no normals: nn == 0)
    const double mc2 = a.min_cos * a.min_cos;
    const double x_max = (double)(a.W - 1) - a.border, y_max = (double)(a.H - 1) - a.border;
    double num[C], best[C], den = 0.0, best_w = -1.0;
#pragma unroll
    for (int c = 0; c < C; c++) num[c] = best[c] = 0.0;
    uint32_t seen = 0;
    for (int v = 0; v < a.V; v++) {
        const double *__restrict__ cam = a.cameras + rn_app::CAMERA_DOUBLES * v;    // uniform
        const double h0 = ((cam[0] * x + cam[1] * y) + cam[2] * z) + cam[3];
        const double h1 = ((cam[4] * x + cam[5] * y) + cam[6] * z) + cam[7];
        const double h2 = ((cam[8] * x + cam[9] * y) + cam[10] * z) + cam[11];
        const double X = h0 / h2, Y = h1 / h2;
        const double dx = cam[12] - x, dy = cam[13] - y, dz = cam[14] - z;
        const double dd = (dx * dx + dy * dy) + dz * dz;
        // every test is a comparison that a NaN fails
        bool ok = h2 > 0.0 && h2 < INFINITY && dd > 0.0 && X >= a.border && X <= x_max &&
                  Y >= a.border && Y <= y_max;
        double w = 1.0;
        if (facing) {
            const double dot = (nx * dx + ny * dy) + nz * dz, q = nn * dd;
            const double dot2 = dot * dot;
            ok = ok && dot > 0.0 && dot2 > mc2 * q;
            w = dot2 / q;
        }
        // a view that does not count reads pixel (0, 0): every load is inside the arrays
        const double Xs = ok ? X : 0.0, Ys = ok ? Y : 0.0;
        if (a.depths) {
            const int xr = (int)rint(Xs), yr = (int)rint(Ys);           // half to even
            const float zf = a.depths[rn_app::depth_index(v, rn_app::pixel_in(yr, a.H) ? yr : 0,
                                                          rn_app::pixel_in(xr, a.W) ? xr : 0,
                                                          a.H, a.W)];
            const double lim = (double)zf + a.tol;
            ok = ok && zf > 0.0f && dd <= lim * lim;
        }
        const double xf = floor(Xs), yf = floor(Ys);
        const double fx = Xs - xf, fy = Ys - yf;
        int x0 = (int)xf, y0 = (int)yf;
        x0 = rn_app::pixel_in(x0, a.W) ? x0 : 0;
        y0 = rn_app::pixel_in(y0, a.H) ? y0 : 0;
        const int x1 = min(x0 + 1, a.W - 1), y1 = min(y0 + 1, a.H - 1);
        double col[C];
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double i00 = a.images[rn_app::image_index(v, y0, x0, c, a.H, a.W, C)],
                         i01 = a.images[rn_app::image_index(v, y0, x1, c, a.H, a.W, C)],
                         i10 = a.images[rn_app::image_index(v, y1, x0, c, a.H, a.W, C)],
                         i11 = a.images[rn_app::image_index(v, y1, x1, c, a.H, a.W, C)];
            const double top = i00 + fx * (i01 - i00), bot = i10 + fx * (i11 - i10);
            col[c] = top + fy * (bot - top);
        }
        if (ok) {
            seen |= 1u << v;
            den = den + w;
            const bool better = w > best_w;         // strictly: the first of equal weights stays
            best_w = better ? w : best_w;
#pragma unroll
            for (int c = 0; c < C; c++) {
                num[c] = num[c] + w * col[c];
                best[c] = better ? col[c] : best[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) {
        const double blend = num[c] / den;
        a.colors[(size_t)i * C + c] = seen ? (float)(a.mode == 0 ? blend : best[c]) : 0.0f;
    }
    a.weight[i] = (float)den;
    a.views[i] = seen;
}

}  // namespace

extern "C" {

int rn_vertex_area_normals(rn_ctx *ctx, int64_t nv, const float *vertices, int64_t nf,
                           const int32_t *faces, const int32_t *offsets, const int32_t *corners,
                           float *normals, void *stream) {
    const rn_app::Verdict v =
        rn_app::normals_args(ctx != nullptr, nv, vertices, nf, faces, offsets, corners, normals);
    if (v == rn_app::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_vertex_area_normals: bad argument (nv %lld, nf %lld)",
                    (long long)nv, (long long)nf);
    if (v == rn_app::EMPTY) return RN_OK;
    hipLaunchKernelGGL(k_vertex_area_normals, dim3((unsigned)((nv + BLOCK - 1) / BLOCK)),
                       dim3(BLOCK), 0, S(stream), nv, vertices, nf, faces, offsets, corners,
                       normals);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_project_colors(rn_ctx *ctx, int64_t n, const float *points, const float *normals,
                      int32_t V, const double *cameras, int32_t H, int32_t W, int32_t C,
                      const float *images, const float *depths, double tol, double min_cos,
                      double border, int32_t mode, float *colors, float *weight, uint32_t *views,
                      void *stream) {
    const rn_app::Verdict v = rn_app::colors_args(ctx != nullptr, n, points, V, cameras, H, W, C,
                                                  images, tol, min_cos, border, mode, colors,
                                                  weight, views);
    if (v == rn_app::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_project_colors: bad argument (n %lld, V %d, H %d, "
                    "W %d, C %d, tol %g, min_cos %g, border %g, mode %d)", (long long)n, (int)V,
                    (int)H, (int)W, (int)C, tol, min_cos, border, (int)mode);
    if (v == rn_app::EMPTY) return RN_OK;
    const ColorArgs a{n, points, normals, V, cameras, H, W, images, depths, tol, min_cos, border,
                      mode, colors, weight, views};
    const dim3 grid((unsigned)((n + BLOCK - 1) / BLOCK));
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(BLOCK), 0, S(stream), a);
    };
    if (C == 1) go(k_project_colors<1>);
    else if (C == 2) go(k_project_colors<2>);
    else if (C == 3) go(k_project_colors<3>);
    else go(k_project_colors<4>);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
