// raynet_holes.inl -- the small holes of an indexed triangle mesh capped: every simple boundary
// loop of at most max_edges half-edges gets a vertex at its centre and a fan of faces (DESIGN.md
// section 25; the definition is in include/raynet_hip.h at rn_mesh_fill_holes).  Included at the
// end of raynet_hip.hip, behind the library's scan (raynet_scan.inl) and the union-find's atomics
// (raynet_components.inl).
//
//   k_holes_init     one thread per vertex: parent[v] = v, the degrees, the loop's edge count and
//                    its bad flag zeroed, out_edge at its largest value; the status word zeroed.
//   k_holes_edges    one thread per half-edge: the boundary test by a gather over the corner list
//                    of the end with fewer corners; a boundary half-edge a -> b adds 1 to
//                    out_deg[a] and in_deg[b], offers itself to out_edge[a] by atomicMin and joins
//                    a and b in the union-find of section 22; one byte flag per half-edge.
//   k_holes_flatten  (the next launch) one thread per vertex: parent[v] = root(v).
//   k_holes_tally    one thread per half-edge: a boundary half-edge adds 1 to the edge count at
//                    parent[a], and 1 to the bad count there if an end fails the degree or the
//                    finiteness test -- the lanes of a wavefront that share a label adding once,
//                    together (section 22's add_by_label).
//   k_holes_flags    one thread per vertex: the scan word of a filled label, (1 << 32) | E, 0
//                    elsewhere; a label adds its part of counts[2..4] to the partial sums of its
//                    workgroup's slot (256 slots, cleared by the launcher).
//   scan_exclusive_u64  (raynet_scan.inl) over the nv words: loops in the high half, faces in the
//                    low half, so one scan numbers the loops and places their faces.
//   k_holes_emit     one thread per vertex: vertex 0 takes the total apart into counts[0..1] and
//                    adds the partial sums up into counts[2..4]; a
//                    filled label walks its loop, E steps, and writes its faces, centre and source.
//
// Integer atomics only, so every word of the workspace is one fixed value whatever the order of the
// threads; no LDS, no floating-point atomic, no sort.  The logic is raynet_holes_args.h's, shared
// with a host program that runs it under the sanitizers; the kernels add the index of the thread
// and the atomics.  No loop waits for another thread and every chase is bounded: the proof is at
// the top of that header.

#include "raynet_holes_args.h"

namespace {

struct HolesArgs {
    rn_hl::Tables tables;
    const float *vertices;
    const int32_t *faces, *offsets, *corners;
    float *new_vertices;
    int32_t *new_faces, *source;
    int64_t *counts;
};

// the atomics policy of rn_hl::mark_edge / tally_edge / flag_vertex on the device: integer
// atomics at agent scope, relaxed
struct HolesAtomics {
    __device__ void add_i32(int32_t *p, int32_t x) const { atomicAdd(p, x); }
    __device__ void min_i32(int32_t *p, int32_t x) const { atomicMin(p, x); }
    __device__ void add_i64(int64_t *p, int64_t x) const {
        atomicAdd((unsigned long long *)p, (unsigned long long)x);
    }
};

__global__ __launch_bounds__(BLOCK) void k_holes_init(HolesArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_hl::vertex_in(v, a.tables.nv);
         v += stride)
        rn_hl::init_vertex(v, a.tables);
}

__global__ __launch_bounds__(BLOCK) void k_holes_edges(HolesArgs a) {
    const HolesAtomics at{};
    const AgentAtomics uf{a.tables.parent};
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t h = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_hl::corner_in(h, a.tables.nf);
         h += stride) {
        if (!rn_hl::mark_edge(at, uf, h, a.faces, a.offsets, a.corners, a.tables)) {
            a.tables.status[0] = 1;
            return;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_holes_flatten(HolesArgs a) {
    const AgentAtomics uf{a.tables.parent};
    const int64_t bound = rn_cc::step_bound(a.tables.nv);
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_hl::vertex_in(v, a.tables.nv);
         v += stride) {
        if (!rn_cc::flatten(uf, (int32_t)v, bound)) {
            a.tables.status[0] = 1;
            return;
        }
    }
}

// (add_by_label is raynet_components.inl's: the lanes of a wavefront that add at the same label add
// once, together.  The rim of a fused surface is one loop of a hundred thousand half-edges, and
// atomics on one word run one after the other.  Every lane of the wavefront reaches it: the loop
// runs on the workgroup's first item.)
__global__ __launch_bounds__(BLOCK) void k_holes_tally(HolesArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t first = blockIdx.x * (int64_t)BLOCK; rn_hl::corner_in(first, a.tables.nf);
         first += stride) {
        const int64_t h = first + threadIdx.x;
        rn_hl::Tally y{-1, false};
        if (rn_hl::corner_in(h, a.tables.nf)) y = rn_hl::tally_of(h, a.vertices, a.faces, a.tables);
        add_by_label(a.tables.edges, (int32_t)y.label, y.label >= 0);
        add_by_label(a.tables.bad, (int32_t)y.label, y.label >= 0 && y.bad);
    }
}

// (the labels' parts go to the partial sums of the workgroup's slot: thousands of labels would
// otherwise meet on the three words of `counts`)
__global__ __launch_bounds__(BLOCK) void k_holes_flags(HolesArgs a) {
    const HolesAtomics at{};
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_hl::vertex_in(v, a.tables.nv);
         v += stride)
        rn_hl::flag_vertex(at, v, a.tables, (int)(blockIdx.x % rn_hl::SLOTS));
}

__global__ __launch_bounds__(BLOCK) void k_holes_emit(HolesArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_hl::vertex_in(v, a.tables.nv);
         v += stride) {
        if (!rn_hl::emit_loop(v, a.vertices, a.faces, a.tables, a.counts, a.new_vertices,
                              a.new_faces, a.source))
            a.tables.status[0] = 1;
    }
}

}  // namespace

extern "C" {

int64_t rn_mesh_fill_holes_workspace_bytes(int64_t nv, int64_t nf) {
    return rn_hl::workspace_bytes(nv, nf);
}

int rn_mesh_fill_holes(rn_ctx *ctx, int64_t nv, const float *vertices, int64_t nf,
                       const int32_t *faces, const int32_t *offsets, const int32_t *corners,
                       int32_t max_edges, float *new_vertices, int32_t *new_faces, int32_t *source,
                       int64_t *counts, void *workspace, void *stream) {
    const rn_hl::Verdict verdict =
        rn_hl::fill_args(ctx != nullptr, nv, vertices, nf, faces, offsets, corners, max_edges,
                         new_vertices, new_faces, source, counts, workspace);
    if (verdict == rn_hl::INVALID)
        return fail(ctx, RN_ERR_INVALID,
                    "rn_mesh_fill_holes: bad argument (nv %lld, nf %lld, max_edges %d)",
                    (long long)nv, (long long)nf, (int)max_edges);
    RN_HIP(ctx, hipMemsetAsync(counts, 0, rn_hl::COUNTS * sizeof(int64_t), S(stream)));
    if (verdict == rn_hl::EMPTY) return RN_OK;
    const rn_hl::Tables t = rn_hl::tables_of(nv, nf, max_edges, workspace);
    const HolesArgs a{t, vertices, faces, offsets, corners, new_vertices, new_faces, source, counts};
    uint64_t *scratch = (uint64_t *)((char *)workspace + rn_hl::ws_scratch(nv, nf));
    RN_HIP(ctx, hipMemsetAsync(t.partial, 0, (size_t)rn_hl::partial_bytes(), S(stream)));
    const dim3 by_vertex((unsigned)rn_hl::blocks(nv, BLOCK)),
               by_edge((unsigned)rn_hl::blocks(3 * nf, BLOCK));
    hipLaunchKernelGGL(k_holes_init, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_holes_edges, by_edge, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_holes_flatten, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_holes_tally, by_edge, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(k_holes_flags, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    const int rc = scan_exclusive_u64(ctx, t.scan, nv, scratch, t.total, S(stream));
    if (rc) return rc;
    hipLaunchKernelGGL(k_holes_emit, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    // the status word comes back: the one wait of the entry
    int32_t status = 0;
    RN_HIP(ctx, hipMemcpyAsync(&status, t.status, sizeof(status), hipMemcpyDeviceToHost, S(stream)));
    RN_HIP(ctx, hipStreamSynchronize(S(stream)));
    if (status != 0)
        return fail(ctx, RN_ERR_STATE,
                    "rn_mesh_fill_holes: a chase or a walk reached what the definition rules out "
                    "(nv %lld, nf %lld): the outputs are not to be used", (long long)nv, (long long)nf);
    return RN_OK;
}

}  // extern "C"
