// raynet_overlap.inl -- which views see a point, how many points every pair of views shares at a
// useful triangulation angle, and what a further view would add to a covering set (DESIGN.md
// section 30; the definitions are in include/raynet_hip.h at rn_view_overlap / rn_view_gain).
// Included near the end of raynet_hip.hip, behind raynet_consistency.inl.
//
//   k_view_overlap  a capped number of blocks, each striding over tiles of 256 points, one lane
//                   per point.  Phase one: the coordinates (and normals) as contiguous fp64
//                   streams, the views in ascending order with wave-uniform camera rows (scalar
//                   loads), the mask of the seeing views in a 64-bit register, one store.  Phase
//                   two: for every view i a 64-bit ballot of its bit -- a wavefront in which no
//                   lane sees i skips i's whole row -- and for every j > i a ballot of both bits,
//                   the pair test per lane only where it is not 0; the popcount of the result's
//                   ballot is ONE count per wavefront and pair, added by one lane to a table of
//                   V (V + 1) / 2 uint32 counters in LDS.  A lane without a point carries mask 0
//                   and stays in every ballot.  At its end a block adds its non-zero counters to
//                   the matrix with 64-bit integer atomics: blocks V (V + 1) / 2 at the most per
//                   launch, whatever n is.
//   k_view_gain     the same tiles over the masks, 8 bytes per point: a ballot per candidate view
//                   of "short and seen by it", lane v keeps view v's count; V + 1 sums per block.
//
// Plain HIP C++: integer counts and integer atomics only, so the result is one fixed array
// whatever order the hardware ran the threads in.  Every fp64 operation of the definition is
// rounded on its own and in the stated order (-ffp-contract=off; the divisions are IEEE; no square
// root anywhere): tests/view_selection_truth.py restates it in np.float64 and the GPU tests ask for
// the same integers.

#include "raynet_overlap_args.h"

namespace {

struct OverlapArgs {
    int64_t n;
    const double *points, *normals;         // [3][n]; normals null for none
    int V;
    const double *cameras;
    int H, W;
    const float *depths;                    // [V][H][W], null for none
    double tol, min_cos, border, lo2, hi2;
    uint64_t *visible;                      // [n]
    unsigned long long *pairs;              // [V][V], the bits of int64
};

static_assert(rn_overlap::BLOCK_SIZE == BLOCK, "the tiles are the library's blocks");

__global__ __launch_bounds__(BLOCK) void k_view_overlap(OverlapArgs a) {
    __shared__ uint32_t counts[rn_overlap::MAX_PAIRS];
    const int V = a.V;
    for (int t = threadIdx.x; t < rn_overlap::pair_count(V); t += BLOCK) counts[t] = 0u;
    __syncthreads();
    const bool first_lane = (threadIdx.x & (WAVE - 1)) == 0;
    const double x_max = (double)(a.W - 1) - a.border, y_max = (double)(a.H - 1) - a.border;
    const double mc2 = a.min_cos * a.min_cos;
    const int64_t tiles = rn_overlap::tiles(a.n);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {              // uniform
        const int64_t i = tile * BLOCK + threadIdx.x;
        const bool in = rn_overlap::point_in(i, a.n);
        const int64_t at = in ? i : 0;          // a lane without a point reads point 0, sets no bit
        const double x = a.points[rn_overlap::coord_index(0, at, a.n)],
                     y = a.points[rn_overlap::coord_index(1, at, a.n)],
                     z = a.points[rn_overlap::coord_index(2, at, a.n)];
        double nx = 0.0, ny = 0.0, nz = 0.0;
        if (a.normals) {                                                            // uniform
            nx = a.normals[rn_overlap::coord_index(0, at, a.n)];
            ny = a.normals[rn_overlap::coord_index(1, at, a.n)];
            nz = a.normals[rn_overlap::coord_index(2, at, a.n)];
        }
        const double nn = (nx * nx + ny * ny) + nz * nz;
        // ---- phase one: the mask
        uint64_t mask = 0;
        for (int v = 0; v < V; v++) {
            const rn_overlap::Sight s = rn_overlap::sees(a.cameras, v, x, y, z, nx, ny, nz, nn, mc2,
                                                         a.H, a.W, a.depths, a.tol, a.border,
                                                         x_max, y_max);
            mask |= (in && s.ok) ? (uint64_t)1 << v : (uint64_t)0;
        }
        if (in) a.visible[i] = mask;
        // ---- phase two: the pairs.  Every lane of the wavefront is here, with or without a point
        for (int vi = 0; vi < V; vi++) {
            const bool sees_i = (mask >> vi) & 1u;
            const uint64_t wave_i = __ballot(sees_i);
            if (wave_i == 0) continue;                                              // uniform
            if (first_lane)
                atomicAdd(&counts[rn_overlap::pair_index(vi, vi, V)], (uint32_t)__popcll(wave_i));
            const rn_overlap::ToCentre ci = rn_overlap::to_centre(a.cameras, vi, x, y, z);
            for (int vj = vi + 1; vj < V; vj++) {
                const bool both = sees_i && ((mask >> vj) & 1u);
                if (__ballot(both) == 0) continue;                                  // uniform
                const rn_overlap::ToCentre cj = rn_overlap::to_centre(a.cameras, vj, x, y, z);
                const uint64_t shared = __ballot(both && rn_overlap::shares(ci, cj, a.lo2, a.hi2));
                if (first_lane && shared != 0)
                    atomicAdd(&counts[rn_overlap::pair_index(vi, vj, V)],
                              (uint32_t)__popcll(shared));
            }
        }
    }
    __syncthreads();
    // ---- the flush: the upper triangle and the diagonal, the non-zero counters only
    for (int t = threadIdx.x; t < V * V; t += BLOCK) {
        const int vi = t / V, vj = t % V;
        if (vj < vi) continue;
        const uint32_t c = counts[rn_overlap::pair_index(vi, vj, V)];
        if (c != 0u) atomicAdd(&a.pairs[rn_overlap::matrix_index(vi, vj, V)], (unsigned long long)c);
    }
}

struct GainArgs {
    int64_t n;
    const uint64_t *visible;
    int V;
    uint64_t chosen;
    int redundancy;
    unsigned long long *gain;               // [V + 1], the bits of int64
};

__global__ __launch_bounds__(BLOCK) void k_view_gain(GainArgs a) {
    __shared__ uint32_t sums[rn_overlap::MAX_VIEWS + 1];
    const int V = a.V;
    if (threadIdx.x <= V) sums[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    const uint64_t candidates = rn_overlap::low_bits(V) & ~a.chosen;
    uint32_t mine = 0u, shorts = 0u;        // lane v: view v's count; every lane: the short points
    const int64_t tiles = rn_overlap::tiles(a.n);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {              // uniform
        const int64_t i = tile * BLOCK + threadIdx.x;
        const bool in = rn_overlap::point_in(i, a.n);
        const uint64_t mask = in ? a.visible[i] : (uint64_t)0;
        const bool is_short = in && rn_overlap::is_short(mask, a.chosen, V, a.redundancy);
        const uint64_t wave_short = __ballot(is_short);
        if (wave_short == 0) continue;                                              // uniform
        shorts += (uint32_t)__popcll(wave_short);
        for (int v = 0; v < V; v++) {
            if (!((candidates >> v) & 1u)) continue;                                // uniform
            const uint32_t c = (uint32_t)__popcll(__ballot(is_short && ((mask >> v) & 1u)));
            mine += lane == v ? c : 0u;
        }
    }
    if (lane < V && mine != 0u) atomicAdd(&sums[lane], mine);
    if (lane == 0 && shorts != 0u) atomicAdd(&sums[V], shorts);
    __syncthreads();
    if (threadIdx.x <= V && sums[threadIdx.x] != 0u)
        atomicAdd(&a.gain[threadIdx.x], (unsigned long long)sums[threadIdx.x]);
}

}  // namespace

extern "C" {

int rn_view_overlap(rn_ctx *ctx, int64_t n, const double *points, const double *normals,
                    int32_t V, const double *cameras, int32_t H, int32_t W, const float *depths,
                    double tol, double min_cos, double border, double cos_lo, double cos_hi,
                    uint64_t *visible, int64_t *pairs, void *stream) {
    const rn_overlap::Verdict verdict = rn_overlap::overlap_args(
        ctx != nullptr, n, points, normals, V, cameras, H, W, depths, tol, min_cos, border, cos_lo,
        cos_hi, visible, pairs);
    if (verdict == rn_overlap::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_view_overlap: bad argument (n %lld, V %d, H %d, W %d, "
                    "tol %g, min_cos %g, border %g, cos_lo %g, cos_hi %g)", (long long)n, (int)V,
                    (int)H, (int)W, tol, min_cos, border, cos_lo, cos_hi);
    if (verdict == rn_overlap::EMPTY) return RN_OK;
    const OverlapArgs a{n, points, normals, V, cameras, H, W, depths, tol, min_cos, border,
                        cos_lo * cos_lo, cos_hi * cos_hi, visible,
                        reinterpret_cast<unsigned long long *>(pairs)};
    hipLaunchKernelGGL(k_view_overlap, dim3((unsigned)rn_overlap::blocks(n)), dim3(BLOCK), 0,
                       S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_view_gain(rn_ctx *ctx, int64_t n, const uint64_t *visible, int32_t V, int64_t chosen,
                 int32_t redundancy, int64_t *gain, void *stream) {
    const rn_overlap::Verdict verdict = rn_overlap::gain_args(ctx != nullptr, n, visible, V,
                                                              redundancy, gain);
    if (verdict == rn_overlap::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_view_gain: bad argument (n %lld, V %d, redundancy %d)",
                    (long long)n, (int)V, (int)redundancy);
    if (verdict == rn_overlap::EMPTY) return RN_OK;
    const GainArgs a{n, visible, V, (uint64_t)chosen, redundancy,
                     reinterpret_cast<unsigned long long *>(gain)};
    hipLaunchKernelGGL(k_view_gain, dim3((unsigned)rn_overlap::blocks(n)), dim3(BLOCK), 0,
                       S(stream), a);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
