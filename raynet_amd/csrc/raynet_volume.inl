// raynet_volume.inl -- the occupancy volume of the MRF, let out of the library: the belief grid
// of an accumulator and its rendering along arbitrary rays.  Included at
// the end of raynet_hip.hip.
//
//   k_occupancy_grid  one thread per voxel: belief = occupancy_to_ray(bias + acc, 0), the very
//                     occupancy k_bp / k_depth would read for that voxel (clamp included), from the
//                     bricked or the [gx][gy][gz] accumulator into a [gx][gy][gz] grid.
//   k_volume_render   one thread per ray: k_traverse's DDA (same set-up, same step arithmetic,
//                     capped at M; the list is never written) with one gather of the belief per
//                     step and the front-to-back products in registers.
//
// Every fp32 operation of the definition is rounded on its own and in the stated order (the
// library is built with -ffp-contract=off): tests/volume_truth.py restates it in np.float32 and
// the GPU tests ask for the same bits.

#include "raynet_volume_args.h"

namespace {

template <bool BRICKED>
__global__ __launch_bounds__(BLOCK) void k_occupancy_grid(Params p, const float *__restrict__ acc,
                                                          float bias, float *belief) {
    const int64_t G = (int64_t)p.gx * p.gy * p.gz;
    for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < G;
         i += (int64_t)gridDim.x * BLOCK) {
        int64_t src = i;
        if (BRICKED) {
            // (only voxels of the grid are addressed: the padding of a partial brick is never read)
            const int z = (int)(i % p.gz), y = (int)((i / p.gz) % p.gy),
                      x = (int)(i / ((int64_t)p.gz * p.gy));
            src = ((((int64_t)(x >> 2) * p.nby + (y >> 2)) * p.nbz + (z >> 2)) << 6) |
                  ((x & 3) << 4) | ((y & 3) << 2) | (z & 3);
        }
        belief[i] = occupancy_to_ray(bias + acc[src], 0.0f);
    }
}

// The DDA of one ray, k_traverse's (ray_tracing.pyx:99-197) operation for operation: the set-up
// below is its set-up, next() its RN_DDA_STEP without the tile.  A function of its own, which
// k_traverse does not call -- that kernel's instructions stay where they are.
struct VolumeDda {
    float tx, ty, tz, td0, td1, td2;
    int pk, pk_last, ux, uy, uz, room_x, room_y, room_z;
    bool active;

    __device__ __forceinline__ void start(const Params &p, const float *s, const float *e) {
        const float EPS = 1e-2f;
        const int g[3] = {p.gx, p.gy, p.gz};
        float ss[3], ee[3], bin[3], ray[3], tm[3], td[3];
        int step[3], cur[3], last[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            ss[i] = s[i] - p.bbox[i];
            ee[i] = e[i] - p.bbox[i];
            bin[i] = (p.bbox[3 + i] - p.bbox[i]) / g[i];
            ray[i] = ee[i] - ss[i];
            step[i] = ray[i] >= 0 ? 1 : -1;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            ss[i] += step[i] * bin[i] * EPS;
            ee[i] -= step[i] * bin[i] * EPS;
            cur[i] = (int)floorf(ss[i] / bin[i]);
            last[i] = (int)floorf(ee[i] / bin[i]);
        }
        active = !(cur[0] < 0 || cur[0] >= g[0] || cur[1] < 0 || cur[1] >= g[1] || cur[2] < 0 ||
                   cur[2] >= g[2]);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            tm[i] = FLT_MAX;
            if (ray[i] != 0) {
                const float c = cur[i] * bin[i];
                float b;
                if (step[i] < 0 && c < ss[i])
                    b = c;
                else
                    b = c + step[i] * bin[i];
                tm[i] = (b - ss[i]) / ray[i];
            }
            td[i] = ray[i] != 0 ? step[i] * bin[i] / ray[i] : FLT_MAX;
        }
        tx = tm[0]; ty = tm[1]; tz = tm[2];
        td0 = td[0]; td1 = td[1]; td2 = td[2];
        pk = pack_voxel(cur[0], cur[1], cur[2]);
        const bool last_in = (unsigned)last[0] < (unsigned)g[0] &&
                             (unsigned)last[1] < (unsigned)g[1] &&
                             (unsigned)last[2] < (unsigned)g[2];
        pk_last = last_in ? pack_voxel(last[0], last[1], last[2]) : -1;
        ux = step[0] * (1 << 20); uy = step[1] * (1 << 10); uz = step[2];
        room_x = step[0] > 0 ? g[0] - 1 - cur[0] : cur[0];
        room_y = step[1] > 0 ? g[1] - 1 - cur[1] : cur[1];
        room_z = step[2] > 0 ? g[2] - 1 - cur[2] : cur[2];
    }
    // leave the voxel `pk` (emitted by the caller) for the next one, or switch the ray off
    __device__ __forceinline__ void next() {
        const bool at_last = pk == pk_last;
        const bool a_ = tx < ty, b_ = tx < tz, c_ = ty < tz;
        const bool mx = a_ & b_, my = !a_ & c_, mxy = mx | my;      // mz = !mxy
        // (one of the three is added; as a sum of masked terms, which is the same integer: a
        // select between the members would make the compiler keep them in an indexed table)
        pk += (mx ? ux : 0) + (my ? uy : 0) + (mxy ? 0 : uz);
        tx += mx ? td0 : 0.0f;
        ty += my ? td1 : 0.0f;
        tz += mxy ? 0.0f : td2;
        room_x -= (int)mx;
        room_y -= (int)my;
        room_z = room_z - 1 + (int)mxy;
        active = !at_last && (room_x | room_y | room_z) >= 0;
    }
};

// entry of a packed voxel in the [gx][gy][gz] belief array; 24-bit multiplies as in lin_xyz
// (coordinates and sizes <= 1024, x gy + y < 2^20)
__device__ __forceinline__ unsigned volume_index(const Params &p, int pk) {
    const unsigned u = (unsigned)pk;
    return mad_u24(mad_u24(u >> 20, (unsigned)p.gy, (u >> 10) & 1023u), (unsigned)p.gz, u & 1023u);
}

// The gathers read the caller's [gx][gy][gz] array: a 4x4x4-bricked copy (what k_bp's gathers
// gain from) was measured and is not faster here, the regrid pass it needs included
// (tools/experiments/volume_render_bricked_gather.patch).
__global__ __launch_bounds__(WAVE) void k_volume_render(Params p, int n,
                                                        const float *__restrict__ starts,
                                                        const float *__restrict__ ends,
                                                        const float *__restrict__ cc,
                                                        const float *__restrict__ axes,
                                                        const float *__restrict__ belief,
                                                        float *out, int64_t out_stride) {
    const int r = blockIdx.x * WAVE + threadIdx.x;
    if (r >= n) return;
    float s[3], e[3];
    for (int i = 0; i < 3; i++) {
        s[i] = starts[3 * (size_t)r + i];
        e[i] = ends[3 * (size_t)r + i];
    }
    VolumeDda dda;
    dda.start(p, s, e);
    // front to back: T the transmittance in front of voxel i, w = o T its weight
    float T = 1.0f, best_w = 0.0f, best_t = 0.0f, sum_w = 0.0f, sum_wt = 0.0f, median = 0.0f;
    bool have_best = false, have_median = false;
    for (int i = 0; i < p.M && dda.active; i++) {
        const float o = belief[volume_index(p, dda.pk)];
        const float t = voxel_distance(p, axes, cc, dda.pk);
        const float w = o * T;
        if (!have_best || w > best_w) {        // the first voxel, then strictly greater only
            best_w = w;
            best_t = t;
            have_best = true;
        }
        sum_wt += w * t;
        sum_w += w;
        T = T * (1.0f - o);
        if (!have_median && T <= 0.5f) {
            median = t;
            have_median = true;
        }
        dda.next();
    }
    // (a ray without voxels: every plane 0.  sum_w is 0 only for such a ray or for a caller's
    // grid of zeros -- the library's own beliefs are >= 1e-4)
    out[rn_volume::out_index(0, out_stride, r)] = best_t;
    out[rn_volume::out_index(1, out_stride, r)] = 1.0f - T;
    out[rn_volume::out_index(2, out_stride, r)] = sum_w > 0.0f ? sum_wt / sum_w : 0.0f;
    out[rn_volume::out_index(3, out_stride, r)] = best_w;
    out[rn_volume::out_index(4, out_stride, r)] = median;
}

}  // namespace

extern "C" {

int rn_occupancy_grid(rn_ctx *ctx, const float *acc, int32_t bricked, float bias,
                      float *belief_out, void *stream) {
    if (rn_volume::grid_args(ctx != nullptr, acc, bricked, belief_out) != rn_volume::LAUNCH)
        return fail(ctx, RN_ERR_INVALID, "rn_occupancy_grid: bad argument");
    const int64_t G = (int64_t)ctx->p.gx * ctx->p.gy * ctx->p.gz;
    if (bricked)
        hipLaunchKernelGGL(k_occupancy_grid<true>, dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream),
                           ctx->p, acc, bias, belief_out);
    else
        hipLaunchKernelGGL(k_occupancy_grid<false>, dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream),
                           ctx->p, acc, bias, belief_out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_volume_render(rn_ctx *ctx, int32_t n, const float *ray_start, const float *ray_end,
                     const float *camera_center, const float *belief, float *out,
                     int64_t out_stride, void *stream) {
    const rn_volume::Verdict v = rn_volume::render_args(ctx != nullptr, n, ray_start, ray_end,
                                                        camera_center, belief, out, out_stride);
    if (v == rn_volume::EMPTY) return RN_OK;
    if (v != rn_volume::LAUNCH)
        return fail(ctx, RN_ERR_INVALID, "rn_volume_render: bad argument (n %d, out_stride %lld)",
                    (int)n, (long long)out_stride);
    int rc = need_axes(ctx);
    if (rc) return rc;
    const dim3 grid((n + WAVE - 1) / WAVE), block(WAVE);
    hipLaunchKernelGGL(k_volume_render, grid, block, 0, S(stream), ctx->p, n, ray_start, ray_end,
                       camera_center, ctx->axes, belief, out, out_stride);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
