// raynet_quadric.inl -- quadric-error placement of the vertices of a clustered mesh (DESIGN.md
// section 28; the definition is in include/raynet_hip.h at rn_mesh_place_quadric).  Included in
// raynet_hip.hip behind raynet_simplify.inl, whose `cluster` and mean positions it consumes.
//
//   k_quadric_clear     one thread per output vertex: its ten sums and its member count zeroed.
//   k_quadric_members   one thread per input vertex: one 64-bit atomicAdd of 1 at its cluster.
//   k_quadric_faces     one thread per input face: the ten fixed-point terms of its plane, by
//                       64-bit atomicAdds, at each distinct cluster among its corners.
//   k_quadric_solve     one thread per output vertex: the 3 x 3 system by L D L^T, the clamp, its
//                       row of positions_out, and the two tallies of `counts`.
//
// Integer atomics only, so every word of the sums is one fixed value whatever the order of the
// threads; no LDS, no floating-point atomic, no sort.  The logic is raynet_quadric_args.h's,
// shared with a host program that runs it under the sanitizers; the kernels add the index of the
// thread and the atomics.

#include "raynet_quadric_args.h"

namespace {

struct QuadricArgs {
    rn_qd::Solve solve;
    rn_qd::Tables tables;
    const float *vertices_in;
    const int32_t *faces_in, *cluster;
    const float *positions_in;
    float *positions_out;
    int64_t *counts;
};

// the atomics policy of rn_qd on the device: 64-bit integer adds at agent scope, relaxed (a
// negative term adds its two's complement)
struct QuadricAtomics {
    __device__ void add_i64(int64_t *p, int64_t x) const {
        atomicAdd((unsigned long long *)p, (unsigned long long)x);
    }
    // 1 to a tally every lane of the launch may add to: the lanes of the wavefront that are here
    // together add their number once (one word takes its atomics one after the other; a lane
    // each, the solve spent nine tenths of its time on the two tallies)
    __device__ void count(int64_t *p) const {
        const unsigned long long here = __ballot(1);
        if ((int)__lane_id() == __ffsll(here) - 1) add_i64(p, (int64_t)__popcll(here));
    }
};

__global__ __launch_bounds__(BLOCK) void k_quadric_clear(QuadricArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t k = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_qd::vertex_in(k, a.tables.nvo);
         k += stride)
        rn_qd::clear(k, a.tables);
}

__global__ __launch_bounds__(BLOCK) void k_quadric_members(QuadricArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_qd::vertex_in(v, a.tables.nv);
         v += stride)
        rn_qd::count_member(QuadricAtomics{}, v, a.cluster, a.tables);
}

__global__ __launch_bounds__(BLOCK) void k_quadric_faces(QuadricArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t f = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_qd::face_in(f, a.tables.nf);
         f += stride)
        rn_qd::add_face(QuadricAtomics{}, f, a.vertices_in, a.faces_in, a.cluster, a.positions_in,
                        a.solve.L, a.tables);
}

__global__ __launch_bounds__(BLOCK) void k_quadric_solve(QuadricArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t k = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_qd::vertex_in(k, a.tables.nvo);
         k += stride)
        rn_qd::solve_vertex(QuadricAtomics{}, k, a.positions_in, a.solve, a.tables,
                            a.positions_out, a.counts);
}

}  // namespace

extern "C" {

int64_t rn_mesh_place_quadric_workspace_bytes(int64_t nv, int64_t nf, int64_t nvo) {
    return rn_qd::workspace_bytes(nv, nf, nvo);
}

int rn_mesh_place_quadric(rn_ctx *ctx, int64_t nv, const float *vertices_in, int64_t nf,
                          const int32_t *faces_in, const int32_t *cluster, int64_t nvo,
                          const float *positions_in, const double cell[3], double regularization,
                          double max_move, float *positions_out, int64_t *counts, void *workspace,
                          void *stream) {
    const rn_qd::Verdict verdict =
        rn_qd::place_args(ctx != nullptr, nv, vertices_in, nf, faces_in, cluster, nvo,
                          positions_in, cell, regularization, max_move, positions_out, counts,
                          workspace);
    if (verdict == rn_qd::INVALID)
        return fail(ctx, RN_ERR_INVALID,
                    "rn_mesh_place_quadric: bad argument (nv %lld, nf %lld, nvo %lld)",
                    (long long)nv, (long long)nf, (long long)nvo);
    RN_HIP(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), S(stream)));
    if (verdict == rn_qd::EMPTY) return RN_OK;
    const rn_qd::Tables t = rn_qd::tables_of(nv, nf, nvo, workspace);
    const QuadricArgs a{rn_qd::solve_of(cell, regularization, max_move), t, vertices_in, faces_in,
                        cluster, positions_in, positions_out, counts};
    const dim3 by_output((unsigned)rn_qd::blocks(nvo, BLOCK)),
               by_vertex((unsigned)rn_qd::blocks(nv, BLOCK)),
               by_face((unsigned)rn_qd::blocks(nf, BLOCK));
    hipLaunchKernelGGL(k_quadric_clear, by_output, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_quadric_members, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    if (nf > 0) {
        hipLaunchKernelGGL(k_quadric_faces, by_face, dim3(BLOCK), 0, S(stream), a);
        RN_LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(k_quadric_solve, by_output, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
