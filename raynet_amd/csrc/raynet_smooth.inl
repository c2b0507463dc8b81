// raynet_smooth.inl -- Taubin's lambda | mu smoothing of an indexed triangle mesh (DESIGN.md section
// 23; the definition is in include/raynet_hip.h at rn_mesh_smooth).  Included at the end of
// raynet_hip.hip.
//
//   k_smooth_ring  one thread per position k of the corner table: the two other vertices of the
//                  face of corners[k], or (-1, -1) where the corner or the face names nothing.
//                  Written once per call, read by every step.
//   k_smooth_step  one thread per vertex: the mean of its row of the ring in fp64, in the row's
//                  order, the move by the step's factor, the clamp against the call's input, one
//                  f32 row stored.  It reads `src` and writes `dst`, two different buffers: no
//                  thread reads what another thread of its launch writes.
//
// Plain loads and stores; no atomics, no LDS, nothing shared between threads.  The logic is
// raynet_smooth_args.h's, shared with a host program that runs it under the sanitizers; the
// kernels add the index of the thread.

#include "raynet_smooth_args.h"

namespace {

struct SmoothArgs {
    int64_t nv, nf;
    const int32_t *faces, *offsets, *corners;
    int32_t *ring;
    const uint8_t *fixed;                   // null for none
    const float *in, *src;
    float *dst;
    double t, max_move;
};

__global__ __launch_bounds__(BLOCK) void k_smooth_ring(SmoothArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t k = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_sm::corner_in(k, a.nf);
         k += stride)
        rn_sm::ring_entry(k, a.nv, a.nf, a.faces, a.corners, a.ring);
}

__global__ __launch_bounds__(BLOCK) void k_smooth_step(SmoothArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_sm::vertex_in(v, a.nv);
         v += stride)
        rn_sm::step_vertex(v, a.nv, a.nf, a.offsets, a.ring, a.fixed, a.in, a.src, a.t,
                           a.max_move, a.dst);
}

}  // namespace

extern "C" {

int64_t rn_mesh_smooth_workspace_bytes(rn_ctx *ctx, int64_t nv, int64_t nf) {
    if (!ctx) return -1;
    if (!rn_sm::sizes_ok(nv, nf)) {
        fail(ctx, RN_ERR_INVALID, "rn_mesh_smooth_workspace_bytes: bad argument (nv %lld, nf %lld)",
             (long long)nv, (long long)nf);
        return -1;
    }
    return rn_sm::workspace_bytes(nv, nf);
}

int rn_mesh_smooth(rn_ctx *ctx, int64_t nv, const float *vertices_in, int64_t nf,
                   const int32_t *faces, const int32_t *offsets, const int32_t *corners,
                   const uint8_t *fixed, int32_t iterations, double lambda, double mu,
                   double max_move, void *workspace, float *vertices_out, void *stream) {
    const rn_sm::Verdict verdict =
        rn_sm::smooth_args(ctx != nullptr, nv, vertices_in, nf, faces, offsets, corners, iterations,
                           lambda, mu, max_move, workspace, vertices_out);
    if (verdict == rn_sm::INVALID)
        return fail(ctx, RN_ERR_INVALID,
                    "rn_mesh_smooth: bad argument (nv %lld, nf %lld, iterations %d, lambda %g, "
                    "mu %g, max_move %g)", (long long)nv, (long long)nf, (int)iterations, lambda,
                    mu, max_move);
    if (verdict == rn_sm::EMPTY) return RN_OK;
    const int64_t L = rn_sm::step_count(iterations, mu);
    if (L == 0) {
        RN_HIP(ctx, hipMemcpyAsync(vertices_out, vertices_in, 12 * (size_t)nv,
                                   hipMemcpyDeviceToDevice, S(stream)));
        return RN_OK;
    }
    int32_t *ring = (int32_t *)workspace;
    float *scratch = (float *)((char *)workspace + rn_sm::scratch_offset(nf));
    SmoothArgs a{nv, nf, faces, offsets, corners, ring, fixed, vertices_in, vertices_in,
                 vertices_out, lambda, max_move};
    if (nf > 0) {
        hipLaunchKernelGGL(k_smooth_ring, dim3((unsigned)rn_sm::blocks(3 * nf, BLOCK)), dim3(BLOCK),
                           0, S(stream), a);
        RN_LAUNCH_CHECK(ctx);
    }
    const dim3 by_vertex((unsigned)rn_sm::blocks(nv, BLOCK));
    for (int64_t i = 1; i <= L; i++) {
        a.t = rn_sm::step_factor(i, lambda, mu);
        a.src = rn_sm::step_source(i, L, vertices_in, scratch, vertices_out);
        a.dst = rn_sm::step_target(i, L, scratch, vertices_out);
        hipLaunchKernelGGL(k_smooth_step, by_vertex, dim3(BLOCK), 0, S(stream), a);
        RN_LAUNCH_CHECK(ctx);
    }
    return RN_OK;
}

}  // extern "C"
