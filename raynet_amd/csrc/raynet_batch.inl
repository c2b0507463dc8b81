// raynet_batch.inl -- a training batch whose rays come from many reference views (DESIGN.md
// section 15).  Included at the end of raynet_hip.hip.
//
//   k_batch_rays     one wavefront per candidate ray, lanes over the D sample points: the ray's
//                    camera comes from a table (a wave-uniform row: scalar loads), so n rays of
//                    any mix of views are ONE launch.  Sample points (K8's arithmetic), the
//                    ground-truth point, the patch centre of every sample point in each of the
//                    ray's N views, and the rejection flags.
//   k_batch_patches  one workgroup per (ray, view): the D patches around those centres, gathered
//                    from the scene's resident channels-last images; every texel is tested
//                    against the image, whatever the centre is.
//
// Every fp32 operation is rounded on its own (-ffp-contract=off) in the order written here:
// tests/batch_truth.py restates both kernels in NumPy and the GPU tests ask for the same bits.

namespace {

constexpr int BATCH_CAMERA_FLOATS = 28;     // P_pinv [4][3] | centre [4] | P [3][4], row-major
static_assert(BATCH_CAMERA_FLOATS == CAMERA_FLOATS, "the schemes read a far view out of the table");
constexpr int BATCH_FLAG_NO_DEPTH = 1, BATCH_FLAG_TARGET_OUTSIDE = 2, BATCH_FLAG_MISSES_BOX = 4,
              BATCH_FLAG_BORDER = 8;

// sample_in_bbox (raynet_kernels.h) line for line, handing out the slab test's verdict as well:
// `misses` = t_near > t_far on the values the swap below then reorders.  A copy, not a shared
// helper: the existing kernels keep their instructions.
__device__ __forceinline__ void batch_sample_in_bbox(const Params &p, int ray_idx,
                                                     const float *__restrict__ P_inv,
                                                     const float *__restrict__ cc, float s[3],
                                                     float e[3], bool &misses) {
    const float px = (float)(ray_idx / p.H);
    const float py = (float)(ray_idx % p.H);
    double o[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double a = 0.0;
        a += (double)(P_inv[3 * r + 0] * px);
        a += (double)(P_inv[3 * r + 1] * py);
        a += (double)P_inv[3 * r + 2] * 1.0;
        o[r] = a;
    }
    float dir[3];
#pragma unroll
    for (int i = 0; i < 3; i++) dir[i] = (float)(o[i] / o[3] - (double)cc[i]);
    float t_near = -INFINITY, t_far = INFINITY;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float t1 = (float)(((double)p.bbox[i] - (double)cc[i]) / (double)dir[i]);
        const float t2 = (float)(((double)p.bbox[3 + i] - (double)cc[i]) / (double)dir[i]);
        t_near = fmaxf(fminf(t1, t2), t_near);
        t_far = fminf(fmaxf(t1, t2), t_far);
    }
    misses = t_near > t_far;
    const float near_mask = (fabsf(t_near) < fabsf(t_far)) ? 1.0f : 0.0f;
    const float tn = t_near * near_mask + t_far * (1 - near_mask);
    const float tf = (1 - near_mask) * t_near + near_mask * t_far;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        s[i] = cc[i] + tn * dir[i];
        e[i] = cc[i] + tf * dir[i];
    }
}

// float -> int32 with the conversion spelled out: NaN -> 0, beyond the range -> the nearest end
__device__ __forceinline__ int32_t batch_to_i32(float x) {
    if (!(x == x)) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (int32_t)0x80000000;
    return (int32_t)x;
}

__global__ __launch_bounds__(BLOCK) void k_batch_rays(
    Params p, int n, const int32_t *__restrict__ view, const int32_t *__restrict__ ray_idxs,
    const float *__restrict__ depth, const float *__restrict__ cams, int V,
    const int32_t *__restrict__ nbr, int N, int ph, int pw, float *points, float *target,
    int32_t *centres, int32_t *flags, int32_t *bad) {
    int lane;
    const int r = ray_of_wave(n, lane);
    if (r < 0) return;
    const int vw = uniform(view[r]), ri = uniform(ray_idxs[r]);
    float4 *row = reinterpret_cast<float4 *>(points) + (size_t)r * p.D;
    int2 *crow = reinterpret_cast<int2 *>(centres) + (size_t)r * N * p.D;
    bool ok = vw >= 0 && vw < V && ri >= 0 && ri < p.H * p.W;
    if (ok)
        for (int j = 0; j < N; j++) {
            const int nv = uniform(nbr[(size_t)vw * N + j]);
            ok = ok && nv >= 0 && nv < V;
        }
    if (!ok) {
        // an index that names no camera / pixel: nothing is read through it; the call fails
        for (int k = lane; k < p.D; k += WAVE) row[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = lane; k < N * p.D; k += WAVE) crow[k] = make_int2(0, 0);
        if (lane == 0) {
            reinterpret_cast<float4 *>(target)[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            flags[r] = 16;
            atomicOr(bad, 1);
        }
        return;
    }
    const float *cam = cams + (size_t)vw * BATCH_CAMERA_FLOATS, *cc = cam + 12;

    // ---- ground-truth point (every lane the same values; lane 0 stores)
    const float u = (float)(ri / p.H), v = (float)(ri % p.H);
    float ray[4];
#pragma unroll
    for (int i = 0; i < 4; i++) ray[i] = (cam[3 * i] * u + cam[3 * i + 1] * v) + cam[3 * i + 2];
    float a[3];
#pragma unroll
    for (int i = 0; i < 3; i++) a[i] = ray[i] / ray[3] - cc[i];
    const float norm = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const float dr = depth[r];
    const bool no_depth = dr == 0.0f || !(fabsf(dr) < INFINITY);
    const float d = no_depth ? 0.0f : dr;
    float t[3];
    bool outside = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        t[i] = a[i] / norm * d + cc[i];
        outside = outside || !(t[i] >= p.bbox[i] && t[i] <= p.bbox[3 + i]);
    }

    // ---- sample points and their patch centres in the ray's N views
    float s[3], e[3];
    bool misses;
    batch_sample_in_bbox(p, ri, cam, cc, s, e, misses);
    const int lo_x = pw / 2, lo_y = ph / 2, hi_x = p.W - pw / 2 - pw % 2, hi_y = p.H - ph / 2 - ph % 2;
    unsigned long long crossing = 0;
    for (int base = 0; base < p.D; base += WAVE) {
        const int k = base + lane;
        const bool live = k < p.D;
        float pt[3];
        plane_point(s, e, live ? k : p.D - 1, p.D, pt);
        if (live) row[k] = make_float4(pt[0], pt[1], pt[2], 1.0f);
        for (int j = 0; j < N; j++) {
            const float *P = cams + (size_t)uniform(nbr[(size_t)vw * N + j]) * BATCH_CAMERA_FLOATS + 16;
            const float qx = ((P[0] * pt[0] + P[1] * pt[1]) + P[2] * pt[2]) + P[3];
            const float qy = ((P[4] * pt[0] + P[5] * pt[1]) + P[6] * pt[2]) + P[7];
            const float qz = ((P[8] * pt[0] + P[9] * pt[1]) + P[10] * pt[2]) + P[11];
            const float x = qx / qz, y = qy / qz;
            const int cx = batch_to_i32(__builtin_rintf(x)), cy = batch_to_i32(__builtin_rintf(y));
            // patches_inside's four inequalities with the sums moved across (no overflow)
            const bool inside = fabsf(x) < INFINITY && fabsf(y) < INFINITY && qz > 0.0f &&
                                cx >= lo_x && cy >= lo_y && cx <= hi_x && cy <= hi_y;
            crossing |= __builtin_amdgcn_ballot_w64(live && !inside);
            if (live) crow[(size_t)j * p.D + k] = make_int2(cx, cy);
        }
    }
    if (lane == 0) {
        reinterpret_cast<float4 *>(target)[r] = make_float4(t[0], t[1], t[2], 1.0f);
        flags[r] = (no_depth ? BATCH_FLAG_NO_DEPTH : 0) | (outside ? BATCH_FLAG_TARGET_OUTSIDE : 0) |
                   (misses ? BATCH_FLAG_MISSES_BOX : 0) | (crossing ? BATCH_FLAG_BORDER : 0);
    }
}

// k_batch_rays with the D sample points where sample_in_range / sample_in_disparity put them
// (SCHEME_RANGE / SCHEME_DISPARITY); target, centres and flags as above on
// those points.  sample_in_disparity's far view is the last of the ray's own neighbour list,
// nbr[view][N - 1]; a ray of it that misses the box gets the camera centre with w = 0 D times and
// BATCH_FLAG_MISSES_BOX.  sample_in_range never sets that flag: the box plays no part in it.
// A second kernel, not a flag in the first: k_batch_rays keeps its instructions
// (profiles/sampling_schemes_isa_identity.txt).
template <int SCHEME>
__global__ __launch_bounds__(BLOCK) void k_batch_rays_scheme(
    Params p, int n, const int32_t *__restrict__ view, const int32_t *__restrict__ ray_idxs,
    const float *__restrict__ depth, const float *__restrict__ cams, int V,
    const int32_t *__restrict__ nbr, int N, int ph, int pw, float *points, float *target,
    int32_t *centres, int32_t *flags, int32_t *bad, float r0, float r1) {
    int lane;
    const int r = ray_of_wave(n, lane);
    if (r < 0) return;
    const int vw = uniform(view[r]), ri = uniform(ray_idxs[r]);
    float4 *row = reinterpret_cast<float4 *>(points) + (size_t)r * p.D;
    int2 *crow = reinterpret_cast<int2 *>(centres) + (size_t)r * N * p.D;
    bool ok = vw >= 0 && vw < V && ri >= 0 && ri < p.H * p.W;
    if (ok)
        for (int j = 0; j < N; j++) {
            const int nv = uniform(nbr[(size_t)vw * N + j]);
            ok = ok && nv >= 0 && nv < V;
        }
    if (!ok) {
        // an index that names no camera / pixel: nothing is read through it; the call fails
        for (int k = lane; k < p.D; k += WAVE) row[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int k = lane; k < N * p.D; k += WAVE) crow[k] = make_int2(0, 0);
        if (lane == 0) {
            reinterpret_cast<float4 *>(target)[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            flags[r] = 16;
            atomicOr(bad, 1);
        }
        return;
    }
    const float *cam = cams + (size_t)vw * BATCH_CAMERA_FLOATS, *cc = cam + 12;

    // ---- ground-truth point (every lane the same values; lane 0 stores)
    const float u = (float)(ri / p.H), v = (float)(ri % p.H);
    float ray[4];
#pragma unroll
    for (int i = 0; i < 4; i++) ray[i] = (cam[3 * i] * u + cam[3 * i + 1] * v) + cam[3 * i + 2];
    float a[3];
#pragma unroll
    for (int i = 0; i < 3; i++) a[i] = ray[i] / ray[3] - cc[i];
    const float norm = sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    const float dr = depth[r];
    const bool no_depth = dr == 0.0f || !(fabsf(dr) < INFINITY);
    const float d = no_depth ? 0.0f : dr;
    float t[3];
    bool outside = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        t[i] = a[i] / norm * d + cc[i];
        outside = outside || !(t[i] >= p.bbox[i] && t[i] <= p.bbox[3 + i]);
    }

    // ---- sample points and their patch centres in the ray's N views
    SchemeRay sr;
    const float *far = cams + (size_t)uniform(nbr[(size_t)vw * N + N - 1]) * BATCH_CAMERA_FLOATS;
    scheme_ray<SCHEME == SCHEME_DISPARITY>(p, SCHEME, r0, r1, ri, cam, cc, far, sr);
    const bool misses = sr.missed;
    const int lo_x = pw / 2, lo_y = ph / 2, hi_x = p.W - pw / 2 - pw % 2, hi_y = p.H - ph / 2 - ph % 2;
    unsigned long long crossing = 0;
    for (int base = 0; base < p.D; base += WAVE) {
        const int k = base + lane;
        const bool live = k < p.D;
        float pt[3];
        scheme_point<SCHEME == SCHEME_DISPARITY>(sr, live ? k : p.D - 1, p.D, pt);
        if (live) row[k] = make_float4(pt[0], pt[1], pt[2], misses ? 0.0f : 1.0f);
        for (int j = 0; j < N; j++) {
            const float *P = cams + (size_t)uniform(nbr[(size_t)vw * N + j]) * BATCH_CAMERA_FLOATS + 16;
            const float qx = ((P[0] * pt[0] + P[1] * pt[1]) + P[2] * pt[2]) + P[3];
            const float qy = ((P[4] * pt[0] + P[5] * pt[1]) + P[6] * pt[2]) + P[7];
            const float qz = ((P[8] * pt[0] + P[9] * pt[1]) + P[10] * pt[2]) + P[11];
            const float x = qx / qz, y = qy / qz;
            const int cx = batch_to_i32(__builtin_rintf(x)), cy = batch_to_i32(__builtin_rintf(y));
            // patches_inside's four inequalities with the sums moved across (no overflow)
            const bool inside = fabsf(x) < INFINITY && fabsf(y) < INFINITY && qz > 0.0f &&
                                cx >= lo_x && cy >= lo_y && cx <= hi_x && cy <= hi_y;
            crossing |= __builtin_amdgcn_ballot_w64(live && !inside);
            if (live) crow[(size_t)j * p.D + k] = make_int2(cx, cy);
        }
    }
    if (lane == 0) {
        reinterpret_cast<float4 *>(target)[r] = make_float4(t[0], t[1], t[2], 1.0f);
        flags[r] = (no_depth ? BATCH_FLAG_NO_DEPTH : 0) | (outside ? BATCH_FLAG_TARGET_OUTSIDE : 0) |
                   (misses ? BATCH_FLAG_MISSES_BOX : 0) | (crossing ? BATCH_FLAG_BORDER : 0);
    }
}

// grid = (n, N): workgroup (r, j) writes out[j][r][D][ph][pw][C] -- channels-last like the
// images, so a patch row is pw * C consecutive floats on both sides.
__global__ __launch_bounds__(BLOCK) void k_batch_patches(
    int n, int D, int H, int W, int C, const float *__restrict__ images, int V,
    const int32_t *__restrict__ view, const int32_t *__restrict__ centres,
    const int32_t *__restrict__ nbr, int N, int ph, int pw, float *out, int32_t *bad) {
    const int r = blockIdx.x, j = blockIdx.y;
    const int vw = view[r];
    const int nv = vw >= 0 && vw < V ? nbr[(size_t)vw * N + j] : -1;
    const bool ok = nv >= 0 && nv < V;
    if (!ok && threadIdx.x == 0) atomicOr(bad, 1);
    const float *img = images + (size_t)(ok ? nv : 0) * H * W * C;
    const int2 *crow = reinterpret_cast<const int2 *>(centres) + ((size_t)r * N + j) * D;
    const int row_floats = pw * C, patch_floats = ph * row_floats;
    float *o = out + ((size_t)j * n + r) * D * patch_floats;
    for (int i = threadIdx.x; i < D * patch_floats; i += BLOCK) {
        const int k = i / patch_floats, rem = i - k * patch_floats;
        const int y = rem / row_floats, xc = rem - y * row_floats;
        const int x = xc / C, c = xc - x * C;
        const int2 ctr = crow[k];
        // 64-bit: a centre may be any int32, the saturated ends included
        const long long py = (long long)ctr.y - ph / 2 + y, px = (long long)ctr.x - pw / 2 + x;
        float val = 0.0f;
        if (ok && py >= 0 && py < H && px >= 0 && px < W) val = img[((size_t)py * W + (size_t)px) * C + c];
        o[i] = val;
    }
}

// the entries' verdict on their index arrays: one int the kernels OR into, read back after the
// launch (the call synchronises its stream: the caller's next step needs the flags anyway)
int batch_indices_ok(rn_ctx *ctx, hipStream_t st, const char *what) {
    RN_HIP(ctx, hipMemcpyAsync(ctx->batch_bad_host, ctx->batch_bad, sizeof(int32_t),
                               hipMemcpyDeviceToHost, st));
    RN_HIP(ctx, hipStreamSynchronize(st));
    if (*ctx->batch_bad_host)
        return fail(ctx, RN_ERR_INVALID, "%s: a view, ray index or neighbour out of range", what);
    return RN_OK;
}

int batch_status_word(rn_ctx *ctx, hipStream_t st) {
    if (!ctx->batch_bad) {
        RN_HIP(ctx, hipMalloc(&ctx->batch_bad, sizeof(int32_t)));
        RN_HIP(ctx, hipHostMalloc(&ctx->batch_bad_host, sizeof(int32_t)));
    }
    RN_HIP(ctx, hipMemsetAsync(ctx->batch_bad, 0, sizeof(int32_t), st));
    return RN_OK;
}

}  // namespace

extern "C" {

int rn_batch_rays(rn_ctx *ctx, int32_t n, const int32_t *view, const int32_t *ray_idxs,
                  const float *depth, const float *cams, int32_t n_views, const int32_t *nbr,
                  int32_t N, int32_t patch_h, int32_t patch_w, float *points, float *target,
                  int32_t *centres, int32_t *flags, void *stream) {
    RN_OPEN(ctx, n, all_set(view, ray_idxs, depth, cams, nbr, points, target, centres, flags) &&
                        n_views >= 1 && N >= 1 && N <= MAX_VIEWS && patch_h >= 1 && patch_w >= 1 &&
                        (int64_t)n * N * ctx->p.D < ((int64_t)1 << 30));
    int rc = batch_status_word(ctx, S(stream));
    if (rc) return rc;
    hipLaunchKernelGGL(k_batch_rays, dim3(ray_blocks(n)), dim3(BLOCK), 0, S(stream), ctx->p, n,
                       view, ray_idxs, depth, cams, n_views, nbr, N, patch_h, patch_w, points,
                       target, centres, flags, ctx->batch_bad);
    RN_LAUNCH_CHECK(ctx);
    return batch_indices_ok(ctx, S(stream), "rn_batch_rays");
}

int rn_batch_rays_scheme(rn_ctx *ctx, int32_t n, const int32_t *view, const int32_t *ray_idxs,
                         const float *depth, const float *cams, int32_t n_views,
                         const int32_t *nbr, int32_t N, int32_t patch_h, int32_t patch_w,
                         const rn_sampling *sampling, float *points, float *target,
                         int32_t *centres, int32_t *flags, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    SchemeArgs sa;
    if (int rc = scheme_args(ctx, sampling, "rn_batch_rays_scheme", sa)) return rc;
    if (sa.id == SCHEME_BBOX)
        return rn_batch_rays(ctx, n, view, ray_idxs, depth, cams, n_views, nbr, N, patch_h, patch_w,
                             points, target, centres, flags, stream);
    RN_OPEN(ctx, n, all_set(view, ray_idxs, depth, cams, nbr, points, target, centres, flags) &&
                        n_views >= 1 && N >= 1 && N <= MAX_VIEWS && patch_h >= 1 && patch_w >= 1 &&
                        (int64_t)n * N * ctx->p.D < ((int64_t)1 << 30));
    int rc = batch_status_word(ctx, S(stream));
    if (rc) return rc;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ray_blocks(n)), dim3(BLOCK), 0, S(stream), ctx->p, n, view,
                           ray_idxs, depth, cams, n_views, nbr, N, patch_h, patch_w, points, target,
                           centres, flags, ctx->batch_bad, sa.r0, sa.r1);
    };
    if (sa.id == SCHEME_DISPARITY) go(k_batch_rays_scheme<SCHEME_DISPARITY>);
    else go(k_batch_rays_scheme<SCHEME_RANGE>);
    RN_LAUNCH_CHECK(ctx);
    return batch_indices_ok(ctx, S(stream), "rn_batch_rays_scheme");
}

int rn_batch_patches(rn_ctx *ctx, int32_t n, const float *images, int32_t n_views, int32_t C,
                     const int32_t *view, const int32_t *centres, const int32_t *nbr, int32_t N,
                     int32_t patch_h, int32_t patch_w, float *patches, void *stream) {
    RN_OPEN(ctx, n, all_set(images, view, centres, nbr, patches) && n_views >= 1 && C >= 1 &&
                        N >= 1 && N <= MAX_VIEWS && patch_h >= 1 && patch_w >= 1 &&
                        (int64_t)ctx->p.D * patch_h * patch_w * C < ((int64_t)1 << 30) &&
                        (int64_t)ctx->p.H * ctx->p.W * C < ((int64_t)1 << 31));
    int rc = batch_status_word(ctx, S(stream));
    if (rc) return rc;
    hipLaunchKernelGGL(k_batch_patches, dim3(n, N), dim3(BLOCK), 0, S(stream), n, ctx->p.D,
                       ctx->p.H, ctx->p.W, C, images, n_views, view, centres, nbr, N, patch_h,
                       patch_w, patches, ctx->batch_bad);
    RN_LAUNCH_CHECK(ctx);
    return batch_indices_ok(ctx, S(stream), "rn_batch_patches");
}

}  // extern "C"
