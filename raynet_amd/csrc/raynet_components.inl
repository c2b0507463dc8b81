// raynet_components.inl -- the connected components of an indexed triangle mesh (DESIGN.md section
// 22; the definition is in include/raynet_hip.h at rn_mesh_components).  Included at the end of
// raynet_hip.hip.
//
// A lock-free union-find over a parent array that IS `labels` (raynet_components_args.h holds the
// logic, shared with a host program that runs it under the sanitizers):
//
//   k_cc_init     labels[v] = v, the counts and the status word zeroed.
//   k_cc_hook     one thread per face over its edges (a, b) and (b, c): find both roots, hang the
//                 larger under the smaller by compare-and-swap.  Every read of `labels` is a relaxed
//                 atomic load at agent scope and every write a compare-and-swap at agent scope that
//                 lowers the word; there is no plain store, no wait on another thread, no LDS.
//   k_cc_flatten  (the next launch) one thread per vertex: labels[v] = root(v), read and written
//                 through the same policy.  The only values a racing store can put into a word are
//                 roots, which are ancestors of it, and roots do not change in this launch.
//   k_cc_count    one thread per vertex and one per face: integer atomicAdd at the label, the
//                 lanes of a wavefront that share a label adding once, together.
//
// Every chase and every retry loop is bounded by nv + 1 steps; a thread that reaches the bound
// writes 1 to the status word and returns, so that a bug ends as an error and not as a hang.

#include "raynet_components_args.h"

namespace {

struct ComponentsArgs {
    int64_t nv, nf;
    const int32_t *faces;
    int32_t *labels, *vertex_counts, *face_counts, *status;    // the last three: null for none
};

// the atomics policy of rn_cc::find / rn_cc::unite on the device: agent scope, relaxed
struct AgentAtomics {
    int32_t *parent;
    __device__ int32_t load(int32_t x) const {
        return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ int32_t cas(int32_t x, int32_t expect, int32_t value) const {
        __hip_atomic_compare_exchange_strong(parent + x, &expect, value, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
    __device__ void store(int32_t x, int32_t value) const {
        __hip_atomic_store(parent + x, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ __launch_bounds__(BLOCK) void k_cc_init(ComponentsArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_cc::vertex_in(v, a.nv);
         v += stride) {
        a.labels[v] = (int32_t)v;
        if (a.vertex_counts) a.vertex_counts[v] = 0;
        if (a.face_counts) a.face_counts[v] = 0;
        if (v == 0 && a.status) a.status[0] = 0;
    }
}

__global__ __launch_bounds__(BLOCK) void k_cc_hook(ComponentsArgs a) {
    const AgentAtomics at{a.labels};
    const int64_t bound = rn_cc::step_bound(a.nv);
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t f = blockIdx.x * (int64_t)BLOCK + threadIdx.x; f < a.nf; f += stride) {
        const int64_t i0 = a.faces[rn_cc::face_index(f, 0)], i1 = a.faces[rn_cc::face_index(f, 1)],
                      i2 = a.faces[rn_cc::face_index(f, 2)];
        if (!rn_cc::face_counts_in(a.nv, i0, i1, i2)) continue;
        const bool ok = rn_cc::unite(at, (int32_t)i0, (int32_t)i1, bound) &&
                        rn_cc::unite(at, (int32_t)i1, (int32_t)i2, bound);
        if (!ok) {
            if (a.status) a.status[0] = 1;
            return;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_cc_flatten(ComponentsArgs a) {
    const AgentAtomics at{a.labels};
    const int64_t bound = rn_cc::step_bound(a.nv);
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t v = blockIdx.x * (int64_t)BLOCK + threadIdx.x; rn_cc::vertex_in(v, a.nv);
         v += stride) {
        if (!rn_cc::flatten(at, (int32_t)v, bound)) {
            if (a.status) a.status[0] = 1;
            return;
        }
    }
}

// atomicAdd of 1 at counts[label] for every lane with `counted`, the lanes of a wavefront that add
// at the same label adding once, together: nearly all faces of a mesh lie in one component, and
// a million atomics on one word run one after the other.  Every lane of the wavefront calls this
// (the callers' loops have uniform trip counts); each round retires the first pending lane and
// every lane with its label, so there are at most 64.  The sums are integers: exact in any order.
__device__ void add_by_label(int32_t *counts, int32_t label, bool counted) {
    unsigned long long pending = __ballot(counted);
    for (int round = 0; round < 64 && pending; round++) {
        const int leader = __ffsll(pending) - 1;
        const int32_t theirs = __shfl(label, leader);
        const unsigned long long same = __ballot(counted && label == theirs);
        if ((int)__lane_id() == leader) atomicAdd(counts + theirs, (int32_t)__popcll(same));
        pending &= ~same;
    }
}

__global__ __launch_bounds__(BLOCK) void k_cc_count(ComponentsArgs a) {
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    const int64_t n = a.nv > a.nf ? a.nv : a.nf;
    // (the loop runs on the workgroup's first item: the same trips for every lane)
    for (int64_t first = blockIdx.x * (int64_t)BLOCK; first < n; first += stride) {
        const int64_t i = first + threadIdx.x;
        if (a.vertex_counts) {
            const bool in = rn_cc::vertex_in(i, a.nv);
            const int64_t r = in ? a.labels[i] : 0;
            add_by_label(a.vertex_counts, (int32_t)r, in && rn_cc::vertex_in(r, a.nv));
        }
        if (a.face_counts) {
            bool in = i < a.nf;
            const int64_t i0 = in ? a.faces[rn_cc::face_index(i, 0)] : 0,
                          i1 = in ? a.faces[rn_cc::face_index(i, 1)] : 0,
                          i2 = in ? a.faces[rn_cc::face_index(i, 2)] : 0;
            in = in && rn_cc::face_counts_in(a.nv, i0, i1, i2);
            const int64_t r = in ? a.labels[i0] : 0;
            add_by_label(a.face_counts, (int32_t)r, in && rn_cc::vertex_in(r, a.nv));
        }
    }
}

}  // namespace

extern "C" {

int rn_mesh_components(rn_ctx *ctx, int64_t nv, int64_t nf, const int32_t *faces,
                       int32_t *labels, int32_t *vertex_counts, int32_t *face_counts,
                       int32_t *status, void *stream) {
    const rn_cc::Verdict verdict = rn_cc::components_args(ctx != nullptr, nv, nf, faces, labels);
    if (verdict == rn_cc::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_mesh_components: bad argument (nv %lld, nf %lld)",
                    (long long)nv, (long long)nf);
    if (verdict == rn_cc::EMPTY) return RN_OK;
    const ComponentsArgs a{nv, nf, faces, labels, vertex_counts, face_counts, status};
    const dim3 by_vertex((unsigned)rn_cc::blocks(nv, BLOCK)),
               by_face((unsigned)rn_cc::blocks(nf, BLOCK)),
               by_both((unsigned)rn_cc::blocks(nv > nf ? nv : nf, BLOCK));
    hipLaunchKernelGGL(k_cc_init, by_vertex, dim3(BLOCK), 0, S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    if (nf > 0) {
        hipLaunchKernelGGL(k_cc_hook, by_face, dim3(BLOCK), 0, S(stream), a);
        RN_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(k_cc_flatten, by_vertex, dim3(BLOCK), 0, S(stream), a);
        RN_LAUNCH_CHECK(ctx);
    }
    if (vertex_counts || face_counts) {
        hipLaunchKernelGGL(k_cc_count, by_both, dim3(BLOCK), 0, S(stream), a);
        RN_LAUNCH_CHECK(ctx);
    }
    return RN_OK;
}

}  // extern "C"
