// raynet_views_args.h -- what a set of views makes of a 3-D point: which of them see it, at which
// pixel and with what weight.  The per-view step of rn_project_colors, which the bake of an atlas
// calls (observe) and whose projection rn_tsdf_integrate shares (project; raynet_fusion.inl); the
// definitions are in include/raynet_hip.h (DESIGN.md sections 20, 21 and 27).  k_project_colors
// (raynet_appearance.inl) alone keeps the step written out, for its speed's sake.  Host-only and
// free of HIP, so that it compiles into a stand-alone program (tests/views_args_main.cpp, built
// with the address and undefined-behaviour sanitizers by tests/test_views_cpu.py); the functions
// are constexpr only so that the device may call them, and forced inline.
// raynet_appearance_args.h and raynet_fusion_args.h import the names they use into their own
// namespace with using-declarations.
//
// Every fp64 operation is rounded on its own and in the stated order (-ffp-contract=off; the
// divisions are IEEE; no square root): tests/appearance_truth.py restates them in np.float64.
// Every image and depth load goes through image_index / map_index with pixel_in-guarded
// coordinates: a view that does not count reads pixel (0, 0).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rn_view {

constexpr int CAMERA_DOUBLES = 15;      // P [3][4] row-major | centre [3]

// pixel (view, y, x) of a [V][H][W] map, channel c of a [V][H][W][C] image
constexpr size_t map_index(int v, int y, int x, int H, int W) {
    return ((size_t)v * (size_t)H + (size_t)y) * (size_t)W + (size_t)x;
}
constexpr size_t image_index(int v, int y, int x, int c, int H, int W, int C) {
    return map_index(v, y, x, H, W) * (size_t)C + (size_t)c;
}
// a pixel coordinate of a view that counts lies in [0, extent - 1]; everything else reads pixel 0
constexpr bool pixel_in(int at, int extent) { return at >= 0 && at < extent; }

// the four neighbours i<row><column> at the fractions (fx, fy): along x first, then along y
constexpr double bilerp(double i00, double i01, double i10, double i11, double fx, double fy) {
    const double top = i00 + fx * (i01 - i00), bot = i10 + fx * (i11 - i10);
    return top + fy * (bot - top);
}

// ---- one view of one point: the pixel (X, Y), the vector to the centre, its squared length, and
// whether the point lies in front of the camera, off its centre and inside the image less the
// border.  x_max = (W - 1) - border, y_max = (H - 1) - border ----
struct Projection {
    double X, Y, dx, dy, dz, dd;
    bool ok;
};
__attribute__((always_inline)) constexpr Projection project(const double *cam,
                                                            double x, double y, double z,
                                                            double border, double x_max,
                                                            double y_max) {
    const double h0 = ((cam[0] * x + cam[1] * y) + cam[2] * z) + cam[3];
    const double h1 = ((cam[4] * x + cam[5] * y) + cam[6] * z) + cam[7];
    const double h2 = ((cam[8] * x + cam[9] * y) + cam[10] * z) + cam[11];
    const double X = h0 / h2, Y = h1 / h2;
    const double dx = cam[12] - x, dy = cam[13] - y, dz = cam[14] - z;
    const double dd = (dx * dx + dy * dy) + dz * dz;
    // every test is a comparison that a NaN fails
    const bool ok = h2 > 0.0 && h2 < INFINITY && dd > 0.0 && X >= border && X <= x_max &&
                    Y >= border && Y <= y_max;
    return Projection{X, Y, dx, dy, dz, dd, ok};
}

// ---- all views of one point: rn_project_colors's definition on an fp64 point and normal ----
struct Views {
    int V;
    const double *cameras;                  // [V][CAMERA_DOUBLES]
    int H, W;
    const float *images, *depths;           // [V][H][W][C]; [V][H][W], null for none
    double tol, min_cos, border;
    int mode;                               // 0: the blend, 1: the best view
};
template <int C>
struct Observation {
    float color[C], weight;
    uint32_t views;
};
// The views in ascending order: projection, the in-view, facing and occlusion tests, a bilinear
// fetch of C channels, the blend or the best view.  A zero normal: no facing test, weight 1.
template <int C>
__attribute__((always_inline)) constexpr Observation<C> observe(const Views &a, double x, double y,
                                                                double z, double nx, double ny,
                                                                double nz) {
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const bool facing = nn > 0.0;                       // (no normals: nn == 0)
    const double mc2 = a.min_cos * a.min_cos;
    const double x_max = (double)(a.W - 1) - a.border, y_max = (double)(a.H - 1) - a.border;
    double num[C] = {}, best[C] = {}, den = 0.0, best_w = -1.0;
    uint32_t seen = 0;
    for (int v = 0; v < a.V; v++) {
        const Projection p = project(a.cameras + CAMERA_DOUBLES * v, x, y, z, a.border, x_max,
                                     y_max);                                    // uniform
        bool ok = p.ok;
        double w = 1.0;
        if (facing) {
            const double dot = (nx * p.dx + ny * p.dy) + nz * p.dz, q = nn * p.dd;
            const double dot2 = dot * dot;
            ok = ok && dot > 0.0 && dot2 > mc2 * q;
            w = dot2 / q;
        }
        // a view that does not count reads pixel (0, 0): every load is inside the arrays
        const double Xs = ok ? p.X : 0.0, Ys = ok ? p.Y : 0.0;
        if (a.depths) {
            const int xr = (int)std::rint(Xs), yr = (int)std::rint(Ys);         // half to even
            const float zf = a.depths[map_index(v, pixel_in(yr, a.H) ? yr : 0,
                                                pixel_in(xr, a.W) ? xr : 0, a.H, a.W)];
            const double lim = (double)zf + a.tol;
            ok = ok && zf > 0.0f && p.dd <= lim * lim;
        }
        const double xf = std::floor(Xs), yf = std::floor(Ys);
        const double fx = Xs - xf, fy = Ys - yf;
        int x0 = (int)xf, y0 = (int)yf;
        x0 = pixel_in(x0, a.W) ? x0 : 0;
        y0 = pixel_in(y0, a.H) ? y0 : 0;
        const int x1 = std::min(x0 + 1, a.W - 1), y1 = std::min(y0 + 1, a.H - 1);
        double col[C] = {};
        for (int c = 0; c < C; c++)
            col[c] = bilerp(a.images[image_index(v, y0, x0, c, a.H, a.W, C)],
                            a.images[image_index(v, y0, x1, c, a.H, a.W, C)],
                            a.images[image_index(v, y1, x0, c, a.H, a.W, C)],
                            a.images[image_index(v, y1, x1, c, a.H, a.W, C)], fx, fy);
        if (ok) {
            seen |= 1u << v;
            den = den + w;
            const bool better = w > best_w;         // strictly: the first of equal weights stays
            best_w = better ? w : best_w;
            for (int c = 0; c < C; c++) {
                num[c] = num[c] + w * col[c];
                best[c] = better ? col[c] : best[c];
            }
        }
    }
    Observation<C> o{};
    for (int c = 0; c < C; c++) {
        const double blend = num[c] / den;
        o.color[c] = seen ? (float)(a.mode == 0 ? blend : best[c]) : 0.0f;
    }
    o.weight = (float)den;
    o.views = seen;
    return o;
}

}  // namespace rn_view
