// raynet_simplify.inl -- vertex clustering of an indexed triangle mesh on a uniform grid (DESIGN.md
// section 24; the definition is in include/raynet_hip.h at rn_mesh_simplify).  Included at the end
// of raynet_hip.hip, behind the library's scan (raynet_scan.inl).
//
//   k_simplify_clear          one thread per cell: the three sums and the count zeroed, rep at its
//                             largest value.
//   k_simplify_bin            one thread per vertex: its cell (or -1) into the workspace, its flag
//                             cleared, and for the binned vertices atomicMin on rep, an integer
//                             atomicAdd on n and three 64-bit atomicAdds on the fixed-point sums --
//                             the lanes of a wavefront that share a cell adding once, together.
//   k_simplify_face_flags     one thread per face: the kept flag into the scan array, and 1 at the
//                             smallest vertex of each of its three clusters (plain stores of the
//                             same value: the race is benign).
//   scan_exclusive_u64        (raynet_scan.inl) over the faces, then over the vertices; the totals
//                             are `counts`.
//   k_simplify_emit_vertices  one thread per vertex: cluster[v]; the smallest vertex of a used
//                             cluster writes the cluster's row of vertices_out and source.
//   k_simplify_emit_faces     one thread per face: a kept face's row of faces_out.
//
// Integer atomics only, so every word of the table is one fixed value whatever the order of the
// threads; no LDS, no floating-point atomic, no sort.  The logic is raynet_simplify_args.h's,
// shared with a host program that runs it under the sanitizers; the kernels add the index of the
// thread, the atomics, and in the binning the sums within a wavefront.

#include "raynet_simplify_args.h"

namespace {

struct SimplifyArgs {
    rn_sp::Grid grid;
    rn_sp::Tables tables;
    const float *vertices_in;
    const int32_t *faces_in;
    float *vertices_out;
    int32_t *faces_out, *source, *cluster;
    const int64_t *counts;
};

// the atomics policy of rn_sp::bin_vertex on the device: integer atomics at agent scope, relaxed
struct SimplifyAtomics {
    __device__ void min_i32(int32_t *p, int32_t x) const { atomicMin(p, x); }
    __device__ void add_i32(int32_t *p, int32_t x) const { atomicAdd(p, x); }
    __device__ void add_u64(uint64_t *p, uint64_t x) const {
        atomicAdd((unsigned long long *)p, (unsigned long long)x);
    }
};

__global__ __launch_bounds__(BLOCK) void k_simplify_clear(SimplifyArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t c = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_sp::cell_in(c, a.grid.cells);
         c += stride)
        rn_sp::clear_cell(c, a.tables);
}

// The five atomics of rn_sp::add_to_cell for every lane with a cell (p.cell >= 0), the lanes of a
// wavefront that share a cell adding once, together: the vertices of an iso-surface come in the
// lattice's order, so a wavefront's 64 fall into a handful of cells, and atomics on one word run
// one after the other.  Every lane of the wavefront calls this (the caller's loop has uniform trip
// counts); each round retires the first pending lane and every lane of its cell, so there are at
// most 64.  64 fixed-point values of at most 2^21 sum to less than 2^32; the lanes hold ascending
// vertices, so the leader's is the group's smallest.  Integer sums: the same in any grouping.
__device__ void add_by_cell(const rn_sp::Tables &t, const rn_sp::Place &p, int32_t v) {
    const SimplifyAtomics at{};
    const bool binned = p.cell >= 0;
    const int32_t cell = (int32_t)p.cell;
    unsigned long long pending = __ballot(binned);
    for (int round = 0; round < 64 && pending; round++) {
        const int leader = __ffsll(pending) - 1;
        const int32_t theirs = __shfl(cell, leader);
        const bool mine = binned && cell == theirs;
        const unsigned long long same = __ballot(mine);
        uint32_t sx = mine ? (uint32_t)p.w[0] : 0u, sy = mine ? (uint32_t)p.w[1] : 0u,
                 sz = mine ? (uint32_t)p.w[2] : 0u;
#pragma unroll
        for (int reach = 32; reach > 0; reach >>= 1) {
            sx += __shfl_xor(sx, reach);
            sy += __shfl_xor(sy, reach);
            sz += __shfl_xor(sz, reach);
        }
        if ((int)__lane_id() == leader)
            rn_sp::add_to_cell(at, t, theirs, v, (int32_t)__popcll(same), sx, sy, sz);
        pending &= ~same;
    }
}

__global__ __launch_bounds__(BLOCK) void k_simplify_bin(SimplifyArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    // (the loop runs on the workgroup's first item: the same trips for every lane)
    for (int64_t first = blockIdx.x * (int64_t)BLOCK; rn_sp::vertex_in(first, a.tables.nv);
         first += stride) {
        const int64_t v = first + threadIdx.x;
        rn_sp::Place p{-1, {0, 0, 0}};
        if (rn_sp::vertex_in(v, a.tables.nv)) p = rn_sp::place_vertex(v, a.vertices_in, a.grid, a.tables);
        add_by_cell(a.tables, p, (int32_t)v);
    }
}

__global__ __launch_bounds__(BLOCK) void k_simplify_face_flags(SimplifyArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t f = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_sp::face_in(f, a.tables.nf);
         f += stride)
        rn_sp::flag_face(f, a.faces_in, a.tables, a.grid.cells);
}

__global__ __launch_bounds__(BLOCK) void k_simplify_emit_vertices(SimplifyArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_sp::vertex_in(v, a.tables.nv);
         v += stride)
        rn_sp::emit_vertex(v, a.vertices_in, a.grid, a.tables, a.counts, a.vertices_out, a.source,
                           a.cluster);
}

__global__ __launch_bounds__(BLOCK) void k_simplify_emit_faces(SimplifyArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t f = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_sp::face_in(f, a.tables.nf);
         f += stride)
        rn_sp::emit_face(f, a.faces_in, a.tables, a.grid.cells, a.faces_out);
}

}  // namespace

extern "C" {

int64_t rn_mesh_simplify_workspace_bytes(int64_t nv, int64_t nf, const int32_t dims[3]) {
    return rn_sp::workspace_bytes(nv, nf, dims);
}

int rn_mesh_simplify(rn_ctx *ctx, int64_t nv, const float *vertices_in, int64_t nf,
                     const int32_t *faces_in, const double origin[3], const double cell[3],
                     const int32_t dims[3], float *vertices_out, int32_t *faces_out,
                     int32_t *source, int32_t *cluster, int64_t *counts, void *workspace,
                     void *stream) {
    const rn_sp::Verdict verdict =
        rn_sp::simplify_args(ctx != nullptr, nv, vertices_in, nf, faces_in, origin, cell, dims,
                             vertices_out, faces_out, counts, workspace);
    if (verdict == rn_sp::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_mesh_simplify: bad argument (nv %lld, nf %lld)",
                    (long long)nv, (long long)nf);
    RN_HIP(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), S(stream)));
    if (verdict == rn_sp::EMPTY) return RN_OK;
    if (nf == 0) {      // no face keeps a cluster: every vertex's is unused
        if (cluster) RN_HIP(ctx, hipMemsetAsync(cluster, 0xff, 4 * (size_t)nv, S(stream)));
        return RN_OK;
    }
    const rn_sp::Grid grid = rn_sp::grid_of(origin, cell, dims);
    const rn_sp::Tables t = rn_sp::tables_of(nv, nf, grid.cells, workspace);
    const SimplifyArgs a{grid, t, vertices_in, faces_in, vertices_out, faces_out, source, cluster,
                         counts};
    uint64_t *scratch = (uint64_t *)((char *)workspace + rn_sp::ws_scratch(nv, nf, grid.cells));
    const dim3 by_cell((unsigned)rn_sp::blocks(grid.cells, BLOCK)),
               by_vertex((unsigned)rn_sp::blocks(nv, BLOCK)),
               by_face((unsigned)rn_sp::blocks(nf, BLOCK));
    hipLaunchKernelGGL(k_simplify_clear, by_cell, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_simplify_bin, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_simplify_face_flags, by_face, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    int rc = scan_exclusive_u64(ctx, t.fscan, nf, scratch, (uint64_t *)(counts + 1), S(stream));
    if (rc) return rc;
    rc = scan_exclusive_u64(ctx, t.vscan, nv, scratch, (uint64_t *)counts, S(stream));
    if (rc) return rc;
    hipLaunchKernelGGL(k_simplify_emit_vertices, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_simplify_emit_faces, by_face, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
