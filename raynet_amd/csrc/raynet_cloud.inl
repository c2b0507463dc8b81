// raynet_cloud.inl -- ground-truth depth of a point cloud: the z-buffer of every view in one
// pass over the points.  Included at the end of raynet_hip.hip.
//
//   k_cloud_zbuffer   one lane per point, a loop over the views: the point is read once, its
//                     projection into every view formed in float64 with every operation rounded on
//                     its own (the library is built with -ffp-contract=off), and the fp32 depth's
//                     bit pattern -- monotone as an unsigned integer for a positive float --
//                     reduced into the view's pixel with an unsigned atomic minimum.
//
// The minimum is exact and order-free, so the buffer does not depend on the launch shape, the
// order of the points or the arrival order of the atomics: tests/cloud_truth.py restates it with
// np.minimum.at and the GPU tests ask for the same bits.

namespace {

constexpr uint32_t CLOUD_EMPTY = 0x7F800000u;      // +inf: the caller's fill value
constexpr int CLOUD_CAMERA_DOUBLES = 21;           // K [3][3] | R [3][3] | t [3], row-major
constexpr int CLOUD_MAX_POINTS = 1 << 30;

// COUNT: also add, once per wavefront, the (point, view) pairs that landed on a pixel
// (counts[0]) and those whose atomic the pre-test skipped (counts[1]).
template <bool COUNT>
__global__ __launch_bounds__(BLOCK) void k_cloud_zbuffer(int n, const float *__restrict__ points,
                                                         int n_views,
                                                         const double *__restrict__ cameras, int H,
                                                         int W, uint32_t *zbuf,
                                                         unsigned long long *counts) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < n;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
        x = (double)points[3 * (size_t)i];
        y = (double)points[3 * (size_t)i + 1];
        z = (double)points[3 * (size_t)i + 2];
    }
    const double inf = (double)INFINITY;
    const size_t view_pixels = (size_t)H * (size_t)W;
    int landed = 0, skipped = 0;
    for (int view = 0; view < n_views; view++) {
        // (uniform addresses: the camera comes through the scalar cache)
        const double *K = cameras + (size_t)view * CLOUD_CAMERA_DOUBLES, *R = K + 9, *t = K + 18;
        const double Xc0 = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
        const double Xc1 = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
        const double Xc2 = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
        const double h0 = (K[0] * Xc0 + K[1] * Xc1) + K[2] * Xc2;
        const double h1 = (K[3] * Xc0 + K[4] * Xc1) + K[5] * Xc2;
        const double h2 = (K[6] * Xc0 + K[7] * Xc1) + K[8] * Xc2;
        const double ru = rint(h0 / h2), rv = rint(h1 / h2);       // half to even, np.rint
        const float z32 = (float)Xc2;
        // every comparison is false for a NaN; an infinite u or v fails the pixel range
        const bool ok = live && h2 > 0.0 && h2 < inf && Xc2 > 0.0 && z32 < INFINITY &&
                        ru >= 0.0 && ru < (double)W && rv >= 0.0 && rv < (double)H;
        if (!ok) continue;
        const uint32_t bits = __float_as_uint(z32);
        uint32_t *cell = zbuf + (size_t)view * view_pixels + (size_t)(int)rv * (size_t)W +
                         (size_t)(int)ru;
        // the stored value only ever decreases, so a stale read (another XCD's L2) is >= the
        // current one: at worst one redundant atomic, never a skipped minimum
        const bool need = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > bits;
        if (need) __hip_atomic_fetch_min(cell, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (COUNT) {
            landed++;
            skipped += need ? 0 : 1;
        }
    }
    if (COUNT) {
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            landed += __shfl_down(landed, off, WAVE);
            skipped += __shfl_down(skipped, off, WAVE);
        }
        if ((threadIdx.x & (WAVE - 1)) == 0 && landed != 0) {
            atomicAdd(&counts[0], (unsigned long long)landed);
            atomicAdd(&counts[1], (unsigned long long)skipped);
        }
    }
}

int cloud_zbuffer(rn_ctx *ctx, int32_t n_points, const float *points, int32_t n_views,
                  const double *cameras, int32_t H, int32_t W, uint32_t *zbuf, uint64_t *counts,
                  bool count, void *stream) {
    RN_OPEN(ctx, n_points, n_points <= CLOUD_MAX_POINTS && n_views >= 0 && H >= 1 && W >= 1 &&
                               (n_views == 0 || all_set(points, cameras, zbuf)) &&
                               (!count || counts != nullptr));
    if (n_views == 0) return RN_OK;
    if (count)
        hipLaunchKernelGGL(k_cloud_zbuffer<true>, dim3(thread_blocks(n_points)), dim3(BLOCK), 0,
                           S(stream), n_points, points, n_views, cameras, H, W, zbuf,
                           reinterpret_cast<unsigned long long *>(counts));
    else
        hipLaunchKernelGGL(k_cloud_zbuffer<false>, dim3(thread_blocks(n_points)), dim3(BLOCK), 0,
                           S(stream), n_points, points, n_views, cameras, H, W, zbuf,
                           (unsigned long long *)nullptr);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // namespace

extern "C" {

int rn_cloud_zbuffer(rn_ctx *ctx, int32_t n_points, const float *points, int32_t n_views,
                     const double *cameras, int32_t H, int32_t W, uint32_t *zbuf, void *stream) {
    return cloud_zbuffer(ctx, n_points, points, n_views, cameras, H, W, zbuf, nullptr, false,
                         stream);
}

int rn_cloud_zbuffer_counted(rn_ctx *ctx, int32_t n_points, const float *points, int32_t n_views,
                             const double *cameras, int32_t H, int32_t W, uint32_t *zbuf,
                             uint64_t *counts, void *stream) {
    return cloud_zbuffer(ctx, n_points, points, n_views, cameras, H, W, zbuf, counts, true, stream);
}

}  // extern "C"
