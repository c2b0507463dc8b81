// raynet_consistency.inl -- what the other views say about a 3-D point: which of them measure
// something at its pixel, which agree with it, and which see past it (the
// definition is in include/raynet_hip.h at rn_points_consistency).  Included at the end of
// raynet_hip.hip.
//
//   k_points_consistency  one thread per point, the three coordinates read as three contiguous
//                         streams, the views in ascending order: projection, the in-view test,
//                         one gather of the depth, the signed distance, three bit masks and the
//                         running sum of the agreeing distances in registers.  The camera rows are
//                         the same for every lane (scalar loads); no LDS, no atomics, nothing
//                         shared between threads, one loop, plain stores.
//
// Plain HIP C++.  Every fp64 operation of the definition is rounded on its own and in the stated
// order (-ffp-contract=off; the divisions are IEEE; no square root anywhere):
// tests/consistency_truth.py restates it in np.float64 and the GPU tests ask for the same bits.

#include "raynet_consistency_args.h"

namespace {

struct ConsistencyArgs {
    int64_t n;
    const double *points;                   // [3][n]
    int V;
    const double *cameras;
    int H, W;
    const float *depths;
    int exclude;                            // the view that is skipped, -1 for none
    double tol_abs, tol_rel, border;
    uint32_t *seen, *agree, *violate;
    float *residual;
};

__global__ __launch_bounds__(BLOCK) void k_points_consistency(ConsistencyArgs a) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (!rn_consistency::point_in(i, a.n)) return;
    const double x = a.points[rn_consistency::coord_index(0, i, a.n)],
                 y = a.points[rn_consistency::coord_index(1, i, a.n)],
                 z = a.points[rn_consistency::coord_index(2, i, a.n)];
    const double x_max = (double)(a.W - 1) - a.border, y_max = (double)(a.H - 1) - a.border;
    uint32_t seen = 0, agree = 0, violate = 0;
    double num = 0.0, cnt = 0.0;
    for (int v = 0; v < a.V; v++) {
        if (v == a.exclude) continue;                                               // uniform
        const rn_view::Projection p = rn_view::project(
            a.cameras + rn_consistency::CAMERA_DOUBLES * v, x, y, z, a.border, x_max, y_max);
        // a view that does not count reads pixel (0, 0): every load is inside the arrays
        const int xr = (int)rint(p.ok ? p.X : 0.0), yr = (int)rint(p.ok ? p.Y : 0.0);  // half to even
        const size_t pixel = rn_consistency::map_index(
            v, rn_consistency::pixel_in(yr, a.H) ? yr : 0, rn_consistency::pixel_in(xr, a.W) ? xr : 0,
            a.H, a.W);
        const double zm = a.depths[pixel];
        const rn_consistency::Vote vote =
            rn_consistency::classify(p.ok, zm, p.dd, a.tol_abs, a.tol_rel);
        const uint32_t bit = 1u << v;
        seen |= vote.measured ? bit : 0u;
        agree |= vote.agrees ? bit : 0u;
        violate |= vote.violates ? bit : 0u;
        if (vote.agrees) {
            num = num + vote.s;
            cnt = cnt + 1.0;
        }
    }
    a.seen[i] = seen;
    a.agree[i] = agree;
    a.violate[i] = violate;
    a.residual[i] = cnt > 0.0 ? (float)(num / cnt) : 0.0f;
}

}  // namespace

extern "C" {

int rn_points_consistency(rn_ctx *ctx, int64_t n, const double *points, int32_t V,
                          const double *cameras, int32_t H, int32_t W, const float *depths,
                          int32_t exclude, double tol_abs, double tol_rel, double border,
                          uint32_t *seen, uint32_t *agree, uint32_t *violate, float *residual,
                          void *stream) {
    const rn_consistency::Verdict verdict = rn_consistency::points_args(
        ctx != nullptr, n, points, V, cameras, H, W, depths, exclude, tol_abs, tol_rel, border,
        seen, agree, violate, residual);
    if (verdict == rn_consistency::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_points_consistency: bad argument (n %lld, V %d, H %d, "
                    "W %d, exclude %d, tol_abs %g, tol_rel %g, border %g)", (long long)n, (int)V,
                    (int)H, (int)W, (int)exclude, tol_abs, tol_rel, border);
    if (verdict == rn_consistency::EMPTY) return RN_OK;
    const ConsistencyArgs a{n, points, V, cameras, H, W, depths, exclude, tol_abs, tol_rel, border,
                            seen, agree, violate, residual};
    hipLaunchKernelGGL(k_points_consistency, dim3((unsigned)rn_consistency::blocks(n, BLOCK)),
                       dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
