// raynet_filters.inl -- the two point-cloud filters between "cloud" and "score" (DESIGN.md
// section 12a).  Included at the end of raynet_hip.hip, after raynet_mesh.inl (mesh_mix64).
//
//   k_voxel_mask   raynet/metrics.py:27-75 + utils/geometry.py:238-240, 315-348: keep the
//                  points inside the closed box whose voxel of the observation mask is 1
//   k_thin_keys    the cell key and the visiting priority of every point
//   k_thin_round   raynet/metrics.py:78-127 (ReduceDensity.filter): one parallel round of the
//                  greedy thinning -- a point is kept iff no earlier-visited kept point lies
//                  within min_dist.  The reference walks the points one after another over a
//                  host KD-tree; the kept set is the lexicographically first maximal
//                  independent set of the graph "distance <= r" under the visiting order, and
//                  rounds of "removed if a kept earlier neighbour exists, kept if every
//                  earlier neighbour is removed" reach exactly that set.
// Everything is float64 like the NumPy code; points are [3][n], planar.

namespace {

constexpr int THIN_UNDECIDED = 0, THIN_KEPT = 1, THIN_REMOVED = 2;
constexpr int THIN_CELL_BITS = 21;
constexpr unsigned long long THIN_GOLDEN = 0x9E3779B97F4A7C15ull;

// box [12]: min xyz | max xyz | step xyz | step / 2 xyz, formed by the caller as NumPy forms
// them from the float32 bounding box.  keep[i] = 1 iff min <= p <= max on every axis and
// mask[ix][iy][iz] == 1 with i = rint((p - min - step / 2) / step) (half to even, np.round),
// clamped to the mask: on the max face of an axis with an even voxel count rint gives the
// count itself (the reference raises IndexError there); below 0 it cannot fall, (p - min -
// step / 2) / step >= -0.5 for p >= min and rint(-0.5) = -0.
__global__ __launch_bounds__(BLOCK) void k_voxel_mask(int n, const double *__restrict__ points,
                                                      const double *__restrict__ box, int A, int B,
                                                      int C, const uint8_t *__restrict__ mask,
                                                      uint8_t *__restrict__ keep) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int shape[3] = {A, B, C};
    int v[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double p = points[(size_t)k * n + i];
        inside = inside && box[k] <= p && p <= box[3 + k];
        const double q = rint((p - box[k] - box[9 + k]) / box[6 + k]);
        // (a NaN or far-away p is outside; the comparisons keep the cast defined)
        v[k] = q >= (double)(shape[k] - 1) ? shape[k] - 1 : (q > 0.0 ? (int)q : 0);
    }
    keep[i] = inside && mask[((size_t)v[0] * B + v[1]) * C + v[2]] == 1 ? 1 : 0;
}

__device__ __forceinline__ unsigned long long thin_key(long long cx, long long cy, long long cz) {
    return ((unsigned long long)(cx + 1) << (2 * THIN_CELL_BITS)) |
           ((unsigned long long)(cy + 1) << THIN_CELL_BITS) | (unsigned long long)(cz + 1);
}

// keys[i] = (cx + 1) << 42 | (cy + 1) << 21 | (cz + 1), c = floor((p - lo) / h);
// priority[i] = position[i] with an explicit order, else
// mix64(mix64(seed + G) + G * (i + 1)), G = 0x9E3779B97F4A7C15, modulo 2^64 (compared unsigned)
__global__ __launch_bounds__(BLOCK) void k_thin_keys(int n, const double *__restrict__ points,
                                                     double lo_x, double lo_y, double lo_z, double h,
                                                     unsigned long long seed_key,
                                                     const int64_t *__restrict__ position,
                                                     unsigned long long *__restrict__ keys,
                                                     unsigned long long *__restrict__ priority) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long cx = (long long)floor((points[i] - lo_x) / h);
    const long long cy = (long long)floor((points[(size_t)n + i] - lo_y) / h);
    const long long cz = (long long)floor((points[2 * (size_t)n + i] - lo_z) / h);
    keys[i] = thin_key(cx, cy, cz);
    priority[i] = position ? (unsigned long long)position[i]
                           : mesh_mix64(seed_key + THIN_GOLDEN * ((unsigned long long)i + 1ull));
}

// One round over the work list (work == NULL: every point), one point per lane.  All arrays are
// in cell order (sorted by key): keys, points [3][n], priority, index (the original index, the
// tie-break of equal priorities).  The 27 cells around a point are nine runs of the sorted
// keys, (cx + dx, cy + dy, cz - 1 .. cz + 1) each: one lower bound, then a scan while the key
// stays in the run.  state is updated in place: it only ever moves from UNDECIDED to its final
// value, so a neighbour's newer (or, from another CU's cache, older) state is equally good;
// the accesses are relaxed agent-scope atomics.  undecided += points still undecided.
__global__ __launch_bounds__(BLOCK) void k_thin_round(int n_work, const int32_t *__restrict__ work,
                                                      int n,
                                                      const unsigned long long *__restrict__ keys,
                                                      const double *__restrict__ points,
                                                      const unsigned long long *__restrict__ priority,
                                                      const int32_t *__restrict__ index, double r2,
                                                      int32_t *state, int32_t *undecided) {
    const int w = blockIdx.x * BLOCK + threadIdx.x;
    bool pending = false;
    if (w < n_work) {
        const int i = work ? work[w] : w;
        if (__hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
            THIN_UNDECIDED) {
            const unsigned long long key = keys[i], pri = priority[i];
            const int idx = index[i];
            const double px = points[i], py = points[(size_t)n + i], pz = points[2 * (size_t)n + i];
            const unsigned long long cell_mask = (1ull << THIN_CELL_BITS) - 1ull;
            // (cx + 1, cy + 1, cz + 1) as stored: all >= 1 and <= 2^21 - 2 (the caller's check)
            const long long kx = (long long)(key >> (2 * THIN_CELL_BITS)),
                            ky = (long long)((key >> THIN_CELL_BITS) & cell_mask),
                            kz = (long long)(key & cell_mask);
            bool removed = false;
            for (int d = 0; d < 9 && !removed; d++) {
                const long long x = kx + d / 3 - 1, y = ky + d % 3 - 1;
                const unsigned long long first = ((unsigned long long)x << (2 * THIN_CELL_BITS)) |
                                                 ((unsigned long long)y << THIN_CELL_BITS) |
                                                 (unsigned long long)(kz - 1);
                const unsigned long long last = first + 2ull;
                int a = 0, b = n;                     // lower bound of `first`
                while (a < b) {
                    const int mid = a + (b - a) / 2;
                    if (keys[mid] < first)
                        a = mid + 1;
                    else
                        b = mid;
                }
                for (int j = a; j < n && keys[j] <= last; j++) {
                    if (j == i) continue;
                    const unsigned long long pj = priority[j];
                    if (!(pj < pri || (pj == pri && index[j] < idx))) continue;      // later
                    const int s = __hip_atomic_load(&state[j], __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
                    if (s == THIN_REMOVED) continue;
                    const double dx = px - points[j], dy = py - points[(size_t)n + j],
                                 dz = pz - points[2 * (size_t)n + j];
                    if (!(dx * dx + dy * dy + dz * dz <= r2)) continue;
                    if (s == THIN_KEPT) {
                        removed = true;
                        break;
                    }
                    pending = true;
                }
            }
            if (removed) pending = false;
            if (!pending)
                __hip_atomic_store(&state[i], removed ? THIN_REMOVED : THIN_KEPT, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // one add per wavefront
    const unsigned long long votes = __ballot(pending);
    if (votes != 0ull && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(undecided, (int)__popcll(votes));
}

constexpr int THIN_MAX_POINTS = 1 << 30;

}  // namespace

extern "C" {

int rn_voxel_mask(rn_ctx *ctx, int32_t n, const double *points, const double *box, int32_t A,
                  int32_t B, int32_t C, const uint8_t *mask, uint8_t *keep, void *stream) {
    RN_OPEN(ctx, n, n <= THIN_MAX_POINTS && A >= 1 && B >= 1 && C >= 1 &&
                        all_set(points, box, mask, keep));
    hipLaunchKernelGGL(k_voxel_mask, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, points,
                       box, A, B, C, mask, keep);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_thin_keys(rn_ctx *ctx, int32_t n, const double *points, double lo_x, double lo_y,
                 double lo_z, double h, int64_t seed, const int64_t *position, int64_t *keys,
                 int64_t *priority, void *stream) {
    RN_OPEN(ctx, n, n <= THIN_MAX_POINTS && h > 0.0 && all_set(points, keys, priority));
    const unsigned long long seed_key = mesh_mix64((unsigned long long)seed + THIN_GOLDEN);
    hipLaunchKernelGGL(k_thin_keys, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, points,
                       lo_x, lo_y, lo_z, h, seed_key, position,
                       reinterpret_cast<unsigned long long *>(keys),
                       reinterpret_cast<unsigned long long *>(priority));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_thin_round(rn_ctx *ctx, int32_t n_work, const int32_t *work, int32_t n,
                  const int64_t *sorted_keys, const double *points, const int64_t *priority,
                  const int32_t *index, double r2, int32_t *state, int32_t *undecided,
                  void *stream) {
    RN_OPEN(ctx, n_work, n >= n_work && n <= THIN_MAX_POINTS && r2 >= 0.0 &&
                             all_set(sorted_keys, points, priority, index, state, undecided));
    hipLaunchKernelGGL(k_thin_round, dim3(thread_blocks(n_work)), dim3(BLOCK), 0, S(stream), n_work,
                       work, n, reinterpret_cast<const unsigned long long *>(sorted_keys), points,
                       reinterpret_cast<const unsigned long long *>(priority), index, r2, state,
                       undecided);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
