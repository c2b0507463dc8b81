// raynet_fusion.inl -- depth maps fused into a truncated signed distance volume over the
// context's grid (the definition is in include/raynet_hip.h at
// rn_tsdf_integrate).  Included at the end of raynet_hip.hip.
//
//   k_tsdf_integrate  one thread per voxel, z fastest (a wavefront's lanes are z-neighbours: the
//                     stores are contiguous and the projections land on neighbouring pixels), the
//                     views in ascending order: projection, the in-view test, one gather of the
//                     depth (and the weight), the signed distance, the running sums in registers.
//                     The camera rows are the same for every lane (scalar loads); no LDS, no
//                     atomics, nothing shared between threads, one loop.
//
// Plain HIP C++.  Every fp64 operation of the definition is rounded on its own and in the stated
// order (-ffp-contract=off; the divisions are IEEE; no sqrt anywhere): tests/fusion_truth.py
// restates it in np.float64 and the GPU tests ask for the same bits.

#include "raynet_fusion_args.h"

namespace {

struct FusionArgs {
    int gx, gy, gz;
    int64_t G;
    const float *axes;                      // the context's tables: x | y | z
    int V;
    const double *cameras;
    int H, W;
    const float *depths, *weights;          // weights: null for 1
    double trunc, border;
    float *tsdf, *weight;
};

__global__ __launch_bounds__(BLOCK) void k_tsdf_integrate(FusionArgs a) {
    const int64_t g = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (!rn_fusion::voxel_in(g, a.G)) return;
    const rn_fusion::Voxel at = rn_fusion::voxel_of(g, a.gy, a.gz);
    const double x = a.axes[rn_fusion::axis_x(at)], y = a.axes[rn_fusion::axis_y(at, a.gx)],
                 z = a.axes[rn_fusion::axis_z(at, a.gx, a.gy)];
    const double x_max = (double)(a.W - 1) - a.border, y_max = (double)(a.H - 1) - a.border;
    double num = 0.0, den = 0.0;
    for (int v = 0; v < a.V; v++) {
        const rn_view::Projection p = rn_view::project(
            a.cameras + rn_fusion::CAMERA_DOUBLES * v, x, y, z, a.border, x_max, y_max);  // uniform
        const double dd = p.dd;
        bool ok = p.ok;
        // a view that does not count reads pixel (0, 0): every load is inside the arrays
        const int xr = (int)rint(ok ? p.X : 0.0), yr = (int)rint(ok ? p.Y : 0.0);   // half to even
        const size_t pixel = rn_fusion::map_index(v, rn_fusion::pixel_in(yr, a.H) ? yr : 0,
                                                  rn_fusion::pixel_in(xr, a.W) ? xr : 0, a.H, a.W);
        const double zm = a.depths[pixel];
        ok = ok && zm > 0.0 && zm < INFINITY;
        double w = 1.0;
        if (a.weights) {
            w = a.weights[pixel];
            ok = ok && w > 0.0 && w < INFINITY;
        }
        const double s = (zm * zm - dd) / (zm + zm);
        ok = ok && s >= -a.trunc;
        const double q = s / a.trunc;
        const double t = q < 1.0 ? q : 1.0;               // min(q, 1); q is no NaN where ok
        if (ok) {
            num = num + w * t;
            den = den + w;
        }
    }
    const bool seen = den > 0.0;
    a.tsdf[g] = seen ? (float)(num / den) : 1.0f;
    a.weight[g] = seen ? (float)den : 0.0f;
}

}  // namespace

extern "C" {

int rn_tsdf_integrate(rn_ctx *ctx, int32_t V, const double *cameras, int32_t H, int32_t W,
                      const float *depths, const float *weights, double trunc, double border,
                      float *tsdf, float *weight, void *stream) {
    const rn_fusion::Verdict verdict = rn_fusion::integrate_args(
        ctx != nullptr, V, cameras, H, W, depths, trunc, border, tsdf, weight);
    if (verdict == rn_fusion::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_tsdf_integrate: bad argument (V %d, H %d, W %d, "
                    "trunc %g, border %g)", (int)V, (int)H, (int)W, trunc, border);
    const int rc = need_axes(ctx);
    if (rc) return rc;
    const Params &p = ctx->p;
    const int64_t G = rn_fusion::voxels(p.gx, p.gy, p.gz);
    const FusionArgs a{p.gx, p.gy, p.gz, G, ctx->axes, V, cameras, H, W, depths, weights, trunc,
                       border, tsdf, weight};
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)rn_fusion::blocks(G, BLOCK)), dim3(BLOCK),
                       0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
