// raynet_scan.inl -- the library's grid-level exclusive scan of 64-bit words.  Included at the end
// of raynet_hip.hip in front of its users, raynet_simplify.inl and raynet_isosurface.inl.
//
//   k_scan_reduce / k_scan_tile
//                   a sum per workgroup, the scan of the sums (the same two kernels, one level up,
//                   as often as the size asks), then every workgroup scans its tile from its own
//                   sum.  Separate launches: no workgroup waits for another.
//   scan_exclusive_u64
//                   the helper that launches them; raynet_scan_args.h sizes its scratch.

#include "raynet_scan_args.h"

namespace {

static_assert(rn_scan::SCAN_TILE == BLOCK, "one entry of the scan per thread of a workgroup");

// inclusive sum over the 64 lanes of a wavefront
__device__ __forceinline__ uint64_t scan_wave_u64(uint64_t x) {
    const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, off);
        x += lane >= off ? y : 0;
    }
    return x;
}

// exclusive sum over the BLOCK threads of a workgroup; *total: the sum of all of them
__device__ __forceinline__ uint64_t scan_block_u64(uint64_t x, uint64_t *total) {
    __shared__ uint64_t wave_sum[WAVES_PER_BLOCK];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const uint64_t incl = scan_wave_u64(x);
    if (lane == WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
        const uint64_t s = wave_sum[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + (incl - x);
}

// sums[b] = the sum of tile b of data[0..n)
__global__ __launch_bounds__(BLOCK) void k_scan_reduce(const uint64_t *__restrict__ data, int64_t n,
                                                       uint64_t *sums) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    uint64_t total;
    scan_block_u64(i < n ? data[i] : 0, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// data[i] <- offsets[tile of i] + the sum of the entries of its tile in front of i.  offsets:
// the scanned sums of k_scan_reduce, or null for a single tile; total_out (single tile only,
// may be null): the sum of everything.
__global__ __launch_bounds__(BLOCK) void k_scan_tile(uint64_t *data, int64_t n,
                                                     const uint64_t *__restrict__ offsets,
                                                     uint64_t *total_out) {
    const int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    uint64_t total;
    const uint64_t excl = scan_block_u64(i < n ? data[i] : 0, &total);
    const uint64_t base = offsets ? offsets[blockIdx.x] : 0;
    if (i < n) data[i] = base + excl;
    if (total_out && threadIdx.x == 0) *total_out = base + total;
}

// The exclusive scan of data[0..n) in place, n >= 1; scratch: rn_scan::scan_scratch_words(n)
// words; total_out (device): the sum of all entries.  Sums wrap modulo 2^64.  Launches only:
// 2 * scan_levels(n) - 1 of them on `stream`, nothing is synchronised.
int scan_exclusive_u64(rn_ctx *ctx, uint64_t *data, int64_t n, uint64_t *scratch,
                       uint64_t *total_out, hipStream_t stream) {
    if (n <= rn_scan::SCAN_TILE) {
        hipLaunchKernelGGL(k_scan_tile, dim3(1), dim3(BLOCK), 0, stream, data, n,
                           (const uint64_t *)nullptr, total_out);
        RN_LAUNCH_CHECK(ctx);
        return RN_OK;
    }
    const int64_t tiles = rn_scan::scan_tiles(n);
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)tiles), dim3(BLOCK), 0, stream,
                       (const uint64_t *)data, n, scratch);
    RN_LAUNCH_CHECK(ctx);
    const int rc = scan_exclusive_u64(ctx, scratch, tiles, scratch + tiles, total_out, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_scan_tile, dim3((unsigned)tiles), dim3(BLOCK), 0, stream, data, n,
                       (const uint64_t *)scratch, (uint64_t *)nullptr);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // namespace
