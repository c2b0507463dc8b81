// raynet_hip.hip -- __global__ kernels and the C ABI (include/raynet_hip.h) of the
// RayNet forward_pass hot path for MI355X / gfx950.  No CPU fallback lives here.
// One translation unit: device helpers and small kernels, the kernel files, the host launch
// layer (raynet_launch.inl), then the ABI entries.
#include "raynet_kernels.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/raynet_hip.h"
#include "raynet_box_policy.h"

using namespace rn;

namespace {

constexpr int BLOCK = 256;               // 4 wavefronts = 4 rays per workgroup
constexpr int RAY_BLOCK = 256;           // threads per workgroup of the wave-per-ray MRF kernels (k_bp, k_depth)
constexpr int WAVES_PER_BLOCK = BLOCK / WAVE;
// The plane sweep's own workgroup size.  The hardware deals consecutive
// workgroups to different CUs, so only a workgroup's own rays share a CU's L1, and the kernel runs
// at the rate its L1s get lines from the L2 -- yet more rays per workgroup do not pay: 384 / 512 /
// 768 / 1024 threads are 22 / 7 / 13 / 36 % slower than 256 at config 2 and 14 / 2 / 14 / 10 % at
// config 4 (profiles/r05_exp_sweep_block.txt; a first run that seemed to gain 11 % had silently
// dropped the folded first BP iteration, whose LDS rows no longer fitted).
constexpr int SWEEP_BLOCK = 256;
constexpr int SWEEP_WAVES = SWEEP_BLOCK / WAVE;
constexpr int NXCD = 8;

// XCD-aware remap: the dispatcher is observed to place block b on XCD b % 8; give
// every XCD one contiguous slice of the ray list so its private L2 sees
// neighbouring rays (speed only -- any placement is correct).
// CHUNK = 0: every XCD gets one contiguous eighth of the list.  CHUNK > 0: chunks of CHUNK
// consecutive work items stay on one XCD and the chunks go round the XCDs -- the XCDs then walk
// the list side by side.  The work per item varies along the list (rays through the middle of
// the box are long, border tiles are empty), so contiguous eighths leave some XCDs idle at the
// end of a launch; what a kernel gains from locality decides its chunk
// (profiles/r03_exp_xcd_chunk.txt): the plane sweep lives off neighbouring rays sharing feature
// rows in L2, the scatter wants the balance.  (The sweep had its eighth until its list loads
// became non-temporal; re-measured after that, chunks of 256 - 1024 rays -- one to four 16 x 16
// pixel tiles -- are 1.5 % faster at config 2 and 6.5 % at config 4, 64 rays are slower, 16384
// much slower.)
constexpr int XCD_CHUNK_SWEEP = 2048 * 64 / 256;      // workgroups: 2048 rays
constexpr int XCD_CHUNK_BP = 256;
// (contiguous eighths until round 6: config 4's k_depth 2.50 -> 2.32 ms per step with chunks of
// 1024 workgroups, config 2 within noise -- profiles/r06_l_variants_probe.txt)
constexpr int XCD_CHUNK_DEPTH = 1024;
constexpr int XCD_CHUNK_SCATTER = 8;
template <int CHUNK = 0>
__device__ __forceinline__ int xcd_block(int b, int nblocks) {
    if (CHUNK > 0) {
        constexpr int C = CHUNK > 0 ? CHUNK : 1;
        const int full = nblocks / (NXCD * C) * (NXCD * C);
        if (b >= full) return b;
        const int xcd = b % NXCD, pos = b / NXCD;
        return ((pos / C) * NXCD + xcd) * C + pos % C;
    }
    const int q = nblocks / NXCD, r = nblocks % NXCD;
    const int xcd = b % NXCD, pos = b / NXCD;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + pos;
}

// the same with a RUN-TIME chunk (work items per XCD group), for launches whose caller sets it
__device__ __forceinline__ int xcd_block_rt(int b, int nblocks, int chunk) {
    const int full = nblocks / (NXCD * chunk) * (NXCD * chunk);
    if (b >= full) return b;
    const int xcd = b % NXCD, pos = b / NXCD;
    return ((pos / chunk) * NXCD + xcd) * chunk + pos % chunk;
}

// Every wave-per-ray kernel is launched as BS threads x ceil(n / (BS / 64)) workgroups, so the
// grid and workgroup sizes follow from the kernel's own argument n: reading gridDim / blockDim
// instead costs a wavefront that lives for ONE ray two more dependent fetches (the hidden
// kernel arguments; blockDim even through the vector memory path) before its first row load:
// k_depth -4 %, k_bp and k_sweep_map -1 % (profiles/r02_exp_wave_startup.txt).
template <int BS = BLOCK, int CHUNK = 0>
__device__ __forceinline__ int ray_of_wave(int n, int &lane, int chunk_rt = 0) {
    constexpr int WPB = BS / WAVE;
    lane = threadIdx.x & (WAVE - 1);
    const int b = chunk_rt > 0 ? xcd_block_rt(blockIdx.x, (n + WPB - 1) / WPB, chunk_rt)
                               : xcd_block<CHUNK>(blockIdx.x, (n + WPB - 1) / WPB);
    // the wave's ray index lives in an SGPR (the compiler cannot see that threadIdx.x >> 6 is
    // wave-uniform): row addresses become scalar base + per-lane 32-bit offset
    const int r = uniform(b * WPB + (int)(threadIdx.x >> 6));
    return r < n ? r : -1;
}

// ------------------------------------------------------------- small kernels
__global__ void k_fill_f32(float *dst, int64_t n, float v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = v;
}
__global__ void k_fill_i32(int32_t *dst, int64_t n, int32_t v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = v;
}
// per-axis centre tables out of the [gx][gy][gz][3] array
__global__ void k_extract_axes(const float *grid, int gx, int gy, int gz, float *axes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < gx)
        axes[i] = grid[((size_t)i * gy * gz) * 3 + 0];
    else if (i < gx + gy)
        axes[i] = grid[((size_t)(i - gx) * gz) * 3 + 1];
    else if (i < gx + gy + gz)
        axes[i] = grid[((size_t)(i - gx - gy)) * 3 + 2];
}
__global__ void k_acc_combine(float *part, int copies, int64_t G, float prior, float *out,
                              int add_prior) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < G;
         i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.0f;
        for (int c = 0; c < copies; c++) {
            s += part[c * G + i];
            part[c * G + i] = 0.0f;
        }
        out[i] = add_prior ? prior + s : s;
    }
}
// the exact arithmetic shortcut next to the expression it replaces (rn_selftest_arith)
__global__ __launch_bounds__(BLOCK) void k_selftest_arith(int n, const float *__restrict__ a,
                                                          float *out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    out[i] = roundf(a[i]);
    out[(size_t)n + i] = round_half_away(a[i]);
}
// round_quotient_fast next to the division it replaces (rn_selftest_quotient); per LANE here,
// where the sweep falls back per wavefront
__global__ __launch_bounds__(BLOCK) void k_selftest_quotient(int n, const float *__restrict__ x,
                                                             const float *__restrict__ d,
                                                             float *out) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    bool sure;
    const float rd = __builtin_amdgcn_rcpf(d[i]);
    const float fast = round_quotient_fast(x[i], rd, sure);
    sure = sure && reciprocal_is_normal(rd);
    out[i] = round_half_away(x[i] / d[i]);
    out[(size_t)n + i] = fast;
    out[2 * (size_t)n + i] = sure ? 1.0f : 0.0f;
}
// the plane sweep's index arithmetic on its own (rn_selftest_feature_offsets): lane = plane, as
// in sweep_coop / sweep_generic
__global__ __launch_bounds__(BLOCK) void k_selftest_offsets(Params p, int n,
                                                            const float *__restrict__ P,
                                                            const float *__restrict__ starts,
                                                            const float *__restrict__ ends,
                                                            int32_t *out) {
    int lane;
    const int r = ray_of_wave(n, lane);
    if (r < 0) return;
    float s[3], e[3];
    for (int i = 0; i < 3; i++) {
        s[i] = starts[3 * r + i];
        e[i] = ends[3 * r + i];
    }
    const float pad_shift = (float)(p.padding - (p.padding - 1) / 2);
    for (int base = 0; base < p.D; base += WAVE) {
        const int k = min(base + lane, p.D - 1);        // (all lanes take part in the ballots)
        float point[3];
        plane_point(s, e, k, p.D, point);
        for (int v = 0; v < p.N; v++) {
            const int generic = feature_offset(p, P + 12 * v, point) / p.F;
            // the cooperative sweep's form (128-byte vectors): byte offset -> vector index
            const int coop = feature_offset_bytes<7>(p, P + 12 * v, point, pad_shift) >> 7;
            if (base + lane < p.D) {
                int32_t *o = out + (((size_t)r * p.N + v) * p.D + k) * 2;
                o[0] = generic;
                o[1] = coop;
            }
        }
    }
}
// the mapping's two exact shortcuts next to the expressions they replace (rn_selftest_mapping)
__global__ __launch_bounds__(BLOCK) void k_selftest_mapping(Params p, int n,
                                                            const float *__restrict__ a,
                                                            const float *__restrict__ b,
                                                            const float *__restrict__ t,
                                                            float *out) {
    extern __shared__ float pos[];
    for (int i = threadIdx.x; i <= p.D; i += BLOCK) pos[i] = 0.0f + i * p.plane_step;
    __syncthreads();
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float y = 1.0f / b[i];
    out[i] = a[i] / b[i];
    out[(size_t)n + i] = markstein_div(a[i], b[i], y);
    out[2 * (size_t)n + i] = markstein_ok(b[i]) && markstein_ok_dividend(a[i]) ? 1.0f : 0.0f;
    const float tc = clampf(t[i], 1e-4f, 1 - 1e-4f);
    out[3 * (size_t)n + i] = (float)plane_index_walk(tc, p.D, p.plane_step);
    out[4 * (size_t)n + i] = (float)plane_index_from_table(pos, tc, p.D);
}
// resident (bricked) accumulator <-> the reference's [gx][gy][gz] array
template <bool TO_GRID>
__global__ void k_acc_regrid(Params p, const float *__restrict__ src, float *dst) {
    const int64_t G = (int64_t)p.gx * p.gy * p.gz;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < G;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % p.gz), y = (int)((i / p.gz) % p.gy), x = (int)(i / ((int64_t)p.gz * p.gy));
        const int64_t b = ((((int64_t)(x >> 2) * p.nby + (y >> 2)) * p.nbz + (z >> 2)) << 6) |
                          ((x & 3) << 4) | ((y & 3) << 2) | (z & 3);
        if (TO_GRID) dst[i] = src[b];
        else dst[b] = src[i];
    }
}
// out[i] = rows[index[i]]: four entries per thread, one 16-byte store -- `out` may be page-locked
// host memory, and whole 256-byte segments per wavefront are what a PCIe write wants
__global__ void k_stitch_rows(int64_t n, const float *__restrict__ rows,
                              const int32_t *__restrict__ index, float *out) {
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int4 ix = reinterpret_cast<const int4 *>(index)[i];
        reinterpret_cast<float4 *>(out)[i] = make_float4(rows[ix.x], rows[ix.y], rows[ix.z], rows[ix.w]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (n4 << 2) + threadIdx.x;
        out[i] = rows[index[i]];
    }
}
__global__ void k_add_scalar(float *a, int64_t n, float v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        a[i] = v + a[i];
}

#include "raynet_prepare.inl"
#include "raynet_mrf.inl"

}  // namespace

// the context and the launchers
#include "raynet_launch.inl"

extern "C" {

// The version string names every compile-time knob the library was built with (all of them
// result-neutral A/B switches or the exact-arithmetic variants of DESIGN.md section 10a; the
// timing-only ablations of earlier rounds live in tools/experiments/ as a patch, not here) and
// whatever extra flags the build script passed (RN_BUILD_EXTRA): tests/test_abi.py holds the
// shipped library to "knobs: none".
#ifndef RN_BUILD_EXTRA
#define RN_BUILD_EXTRA ""
#endif
const char *rn_version(void) {
    static const char v[] = "raynet_hip 0.4 (gfx950) knobs:"
#ifdef RN_EXACT_OCC_EXP
        " RN_EXACT_OCC_EXP"
#endif
#ifdef RN_EXACT_SOFTMAX_EXP
        " RN_EXACT_SOFTMAX_EXP"
#endif
#ifdef RN_EXACT_BP_MATH
        " RN_EXACT_BP_MATH"
#endif
        " | extra:" RN_BUILD_EXTRA;
    return v;
}

const char *rn_last_error(const rn_ctx *ctx) { return ctx ? ctx->err : "null context"; }

int rn_create(const rn_config *cfg, rn_ctx **out) {
    if (!cfg || !out) return RN_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RN_ERR_NO_DEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return RN_ERR_NO_DEVICE;
    if (cfg->M < 1 || cfg->M > MAX_M || cfg->D < 2 || cfg->D > MAX_D || cfg->N < 2 ||
        cfg->N > MAX_VIEWS || cfg->F < 1 || cfg->H < 1 || cfg->W < 1 || cfg->padding < 0)
        return RN_ERR_INVALID;
    for (int i = 0; i < 3; i++)
        if (cfg->grid[i] < 1 || cfg->grid[i] > MAX_GRID_AXIS || !(cfg->bbox[3 + i] > cfg->bbox[i]))
            return RN_ERR_INVALID;
    if ((int64_t)((cfg->grid[0] + 3) / 4) * ((cfg->grid[1] + 3) / 4) * ((cfg->grid[2] + 3) / 4) >=
        ((int64_t)1 << 24))
        return RN_ERR_INVALID;        // accumulator indices are 32-bit
    if ((int64_t)(cfg->H + cfg->padding + 1) * (cfg->W + cfg->padding + 1) * cfg->F >=
        ((int64_t)1 << 29))
        return RN_ERR_INVALID;        // feature vectors are addressed with 32-bit byte offsets
    // (every shape within these limits fits the LDS of a CU: the static_assert at sweep_lds_bytes)
    if (hipSetDevice(cfg->device) != hipSuccess) return RN_ERR_HIP;
    rn_ctx *ctx = new rn_ctx();
    ctx->cfg = *cfg;
    Params &p = ctx->p;
    p.M = cfg->M; p.D = cfg->D; p.N = cfg->N; p.F = cfg->F;
    p.H = cfg->H; p.W = cfg->W; p.padding = cfg->padding;
    p.gx = cfg->grid[0]; p.gy = cfg->grid[1]; p.gz = cfg->grid[2];
    p.nby = (p.gy + 3) / 4; p.nbz = (p.gz + 3) / 4;
    p.plane_step = (1.0f - 0.0f) / (p.D - 1);
    p.Hf = cfg->H + cfg->padding + 1;
    p.Wf = cfg->W + cfg->padding + 1;
    for (int i = 0; i < 6; i++) p.bbox[i] = cfg->bbox[i];
    const char *sm = getenv("RAYNET_HIP_SCATTER_MODE");
    ctx->scatter_mode = sm ? atoi(sm) : -1;
    const char *bs = getenv("RAYNET_HIP_BOX_LEVEL");      // A/B knob: start at this tile shape
    ctx->box.start(bs ? max(0, min(BoxPolicy::LAST, atoi(bs))) : 0,
                   getenv("RAYNET_HIP_BOX_PIN") != nullptr);
    const char *ov = getenv("RAYNET_HIP_OVERLAP");
    ctx->overlap = ov ? (atoi(ov) != 0 ? 1 : 0) : 2;
    ctx->generic_sweep = getenv("RAYNET_HIP_GENERIC_SWEEP") != nullptr;
    const char *rw = getenv("RAYNET_HIP_SWEEP_RAYS_PER_WAVE");
    ctx->sweep_rpw = rw && atoi(rw) == 1 ? 1 : 0;
    if (hipMalloc(&ctx->axes, sizeof(float) * (p.gx + p.gy + p.gz)) != hipSuccess ||
        hipMalloc(&ctx->box_stats, 2 * sizeof(unsigned)) != hipSuccess ||
        hipMalloc(&ctx->scalar_dev, sizeof(float)) != hipSuccess ||
        hipHostMalloc(&ctx->box_stats_host, 2 * sizeof(unsigned)) != hipSuccess ||
        hipMemset(ctx->box_stats, 0, 2 * sizeof(unsigned)) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
        rn_destroy(ctx);                  // frees whatever was created (all null-checked)
        return RN_ERR_HIP;
    }
    ctx->box_stats_host[0] = ctx->box_stats_host[1] = 0;
    *out = ctx;
    return RN_OK;
}

void rn_destroy(rn_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->cfg.device);
    if (ctx->axes) hipFree(ctx->axes);
    if (ctx->box_stats) hipFree(ctx->box_stats);
    if (ctx->scalar_dev) hipFree(ctx->scalar_dev);
    if (ctx->box_stats_host) hipHostFree(ctx->box_stats_host);
    if (ctx->batch_bad) hipFree(ctx->batch_bad);
    if (ctx->range_seg) hipFree(ctx->range_seg);
    if (ctx->batch_bad_host) hipHostFree(ctx->batch_bad_host);
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    if (ctx->aux) hipStreamDestroy(ctx->aux);
    for (int i = 0; i < 2 * ctx->prof_cap; i++) hipEventDestroy(ctx->prof_ev[i]);
    delete[] ctx->prof_ev;
    delete[] ctx->prof_id;
    delete[] ctx->prof_rays;
    delete ctx;
}

int rn_get_options(const rn_ctx *ctx, rn_options *out) {
    if (!ctx || !out) return RN_ERR_INVALID;
    out->scatter_mode = ctx->scatter_mode;
    out->box_level = ctx->box.level0;
    out->box_pin = ctx->box.pin ? 1 : 0;
    out->overlap = ctx->overlap;
    out->generic_sweep = ctx->generic_sweep;
    out->sweep_rays_per_wave = ctx->sweep_rpw;
    return RN_OK;
}

int rn_set_options(rn_ctx *ctx, const rn_options *opt) {
    if (!ctx || !opt) return RN_ERR_INVALID;
    if ((opt->scatter_mode != -1 && opt->scatter_mode != 0 && opt->scatter_mode != 2) ||
        opt->box_level < 0 || opt->box_level > 2 || opt->overlap < 0 || opt->overlap > 2 ||
        (opt->sweep_rays_per_wave != 0 && opt->sweep_rays_per_wave != 1))
        return fail(ctx, RN_ERR_INVALID, "rn_set_options: value out of range");
    ctx->scatter_mode = opt->scatter_mode;
    ctx->box.start(opt->box_level, opt->box_pin != 0);
    ctx->overlap = opt->overlap;
    ctx->generic_sweep = opt->generic_sweep != 0;
    ctx->sweep_rpw = opt->sweep_rays_per_wave;
    return RN_OK;
}

int rn_set_voxel_grid(rn_ctx *ctx, const float *voxel_grid, void *stream) {
    if (!ctx || !voxel_grid) return fail(ctx, RN_ERR_INVALID, "null argument");
    const Params &p = ctx->p;
    const int tot = p.gx + p.gy + p.gz;
    hipLaunchKernelGGL(k_extract_axes, dim3(thread_blocks(tot)), dim3(BLOCK), 0, S(stream),
                       voxel_grid, p.gx, p.gy, p.gz, ctx->axes);
    RN_LAUNCH_CHECK(ctx);
    ctx->have_axes = true;
    return RN_OK;
}

int rn_fill_f32(rn_ctx *ctx, float *dst, int64_t count, float value, void *stream) {
    if (!ctx || (!dst && count)) return fail(ctx, RN_ERR_INVALID, "null argument");
    if (count <= 0) return RN_OK;
    hipLaunchKernelGGL(k_fill_f32, dim3(fill_blocks(count)), dim3(BLOCK), 0, S(stream), dst, count,
                       value);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_fill_i32(rn_ctx *ctx, int32_t *dst, int64_t count, int32_t value, void *stream) {
    if (!ctx || (!dst && count)) return fail(ctx, RN_ERR_INVALID, "null argument");
    if (count <= 0) return RN_OK;
    hipLaunchKernelGGL(k_fill_i32, dim3(fill_blocks(count)), dim3(BLOCK), 0, S(stream), dst, count,
                       value);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_sample_rays(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *P_inv,
                   const float *camera_center, float *ray_start, float *ray_end, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, P_inv, camera_center, ray_start, ray_end));
    hipLaunchKernelGGL(k_sample_rays, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), ctx->p, n,
                       ray_idxs, P_inv, camera_center, ray_start, ray_end);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_sample_points(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *P_inv,
                     const float *camera_center, float *points, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, P_inv, camera_center, points));
    hipLaunchKernelGGL(k_sample_points, dim3(ray_blocks(n)), dim3(BLOCK), 0, S(stream), ctx->p, n,
                       ray_idxs, P_inv, camera_center, points);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_compute_similarities(rn_ctx *ctx, int32_t n, const float *features, const float *P,
                            const float *ray_start, const float *ray_end, float *Sp,
                            void *stream) {
    RN_OPEN(ctx, n, all_set(features, P, ray_start, ray_end, Sp));
    SweepArgs a{n, nullptr, stacked_views(ctx->p, features), P, nullptr, nullptr, ray_start,
                ray_end, nullptr, nullptr, nullptr, Sp, nullptr, nullptr, nullptr};
    launch_sweep<0, false>(ctx, a, true, S(stream));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_voxel_traversal(rn_ctx *ctx, int32_t n, const float *ray_start, const float *ray_end,
                       int32_t *rvi, int32_t *rvc, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_start, ray_end, rvi, rvc));
    {
        ProfScope prof(ctx, RN_K_TRAVERSE, n, S(stream));
        hipLaunchKernelGGL((k_traverse<false>), dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, S(stream),
                           ctx->p, n, (const int32_t *)nullptr, (const float *)nullptr,
                           (const float *)nullptr, ray_start, ray_end, rvi, rvc, 0, (int64_t)0,
                           (float *)nullptr);
    }
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_planes_to_voxels(rn_ctx *ctx, int32_t n, const int32_t *rvi, const int32_t *rvc,
                        const float *ray_start, const float *ray_end, const float *Sp,
                        float *S_new, void *stream) {
    RN_OPEN(ctx, n, all_set(rvi, rvc, ray_start, ray_end, Sp, S_new));
    int rc = need_axes(ctx);
    if (rc) return rc;
    SweepArgs a{n, nullptr, FeatureViews{}, nullptr, nullptr, nullptr, ray_start, ray_end, Sp,
                rvi, rvc, nullptr, S_new, nullptr, nullptr};
    launch_sweep<1, false>(ctx, a, false, S(stream));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_bp_sweep(rn_ctx *ctx, int32_t n, const float *Sv, const int32_t *rvi, const int32_t *rvc,
                const float *acc_in, const float *msgs_in, float *acc_out, float *msgs_out,
                void *stream) {
    RN_OPEN(ctx, n, all_set(Sv, rvi, rvc, acc_in, acc_out, msgs_out));   /* msgs_in == NULL: all-zero messages */
    return launch_bp<false, true>(ctx, n, Sv, rvi, rvc, acc_in, msgs_in, acc_out, msgs_out,
                                  S(stream));
}

int rn_depth_estimation(rn_ctx *ctx, int32_t n, const float *Sv, const int32_t *rvi,
                        const int32_t *rvc, const float *acc, const float *msgs, float *S_new,
                        void *stream) {
    RN_OPEN(ctx, n, all_set(Sv, rvi, rvc, acc, msgs, S_new));
    return launch_depth<false, true>(ctx, n, Sv, rvi, rvc, acc, msgs, nullptr, S_new, nullptr,
                                     S(stream));
}

int rn_mvcnn_similarities(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                          const float *P, const float *P_inv, const float *camera_center,
                          float *Sp, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, Sp));
    SweepArgs a{n, ray_idxs, stacked_views(ctx->p, features), P, P_inv, camera_center, nullptr,
                nullptr, nullptr, nullptr, nullptr, Sp, nullptr, nullptr, nullptr};
    launch_sweep<0, false>(ctx, a, true, S(stream));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mvcnn_depth(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                   const float *P, const float *P_inv, const float *camera_center, float *Sp,
                   float *points, float *depth_map, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, Sp, points, depth_map));
    SweepArgs a{n, ray_idxs, stacked_views(ctx->p, features), P, P_inv, camera_center, nullptr,
                nullptr, nullptr, nullptr, nullptr, Sp, nullptr, depth_map, points};
    launch_sweep<0, false>(ctx, a, true, S(stream));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

// ---- the same three under a sampling scheme (sampling_schemes.py:178-297)
static_assert(RN_SAMPLE_IN_BBOX == SCHEME_BBOX && RN_SAMPLE_IN_RANGE == SCHEME_RANGE &&
              RN_SAMPLE_IN_DISPARITY == SCHEME_DISPARITY, "the header's ids are the kernels'");

int rn_sample_points_scheme(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *P_inv,
                            const float *camera_center, const rn_sampling *sampling,
                            float *points, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    SchemeArgs sa;
    if (int rc = scheme_args(ctx, sampling, "rn_sample_points_scheme", sa)) return rc;
    if (sa.id == SCHEME_BBOX)
        return rn_sample_points(ctx, n, ray_idxs, P_inv, camera_center, points, stream);
    RN_OPEN(ctx, n, all_set(ray_idxs, P_inv, camera_center, points));
    if (sa.id == SCHEME_DISPARITY)
        hipLaunchKernelGGL(k_sample_points_scheme<true>, dim3(ray_blocks(n)), dim3(BLOCK), 0,
                           S(stream), ctx->p, n, ray_idxs, P_inv, camera_center, sa, points);
    else
        hipLaunchKernelGGL(k_sample_points_scheme<false>, dim3(ray_blocks(n)), dim3(BLOCK), 0,
                           S(stream), ctx->p, n, ray_idxs, P_inv, camera_center, sa, points);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mvcnn_similarities_scheme(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs,
                                 const float *features, const float *P, const float *P_inv,
                                 const float *camera_center, const rn_sampling *sampling,
                                 float *Sp, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    SchemeArgs sa;
    if (int rc = scheme_args(ctx, sampling, "rn_mvcnn_similarities_scheme", sa)) return rc;
    if (sa.id == SCHEME_BBOX)
        return rn_mvcnn_similarities(ctx, n, ray_idxs, features, P, P_inv, camera_center, Sp, stream);
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, Sp));
    if (int rc = launch_sweep_scheme(ctx, n, ray_idxs, features, P, P_inv, camera_center, sa, Sp,
                                     nullptr, nullptr, S(stream)))
        return rc;
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mvcnn_depth_scheme(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                          const float *P, const float *P_inv, const float *camera_center,
                          const rn_sampling *sampling, float *Sp, float *points,
                          float *depth_map, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    SchemeArgs sa;
    if (int rc = scheme_args(ctx, sampling, "rn_mvcnn_depth_scheme", sa)) return rc;
    if (sa.id == SCHEME_BBOX)
        return rn_mvcnn_depth(ctx, n, ray_idxs, features, P, P_inv, camera_center, Sp, points,
                              depth_map, stream);
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, Sp, points, depth_map));
    if (int rc = launch_sweep_scheme(ctx, n, ray_idxs, features, P, P_inv, camera_center, sa, Sp,
                                     depth_map, points, S(stream)))
        return rc;
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

static int prefix_api(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                      const float *P, const float *P_inv, const float *cc, int32_t *rvi,
                      int32_t *rvc, float *S_voxel, hipStream_t st) {
    // raynet_fp.py:55-104: traversal (thread per ray), then sweep + mapping (wave per ray)
    {
        ProfScope prof(ctx, RN_K_TRAVERSE, n, st);
        hipLaunchKernelGGL((k_traverse<false>), dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, st, ctx->p,
                           n, ray_idxs, P_inv, cc, (const float *)nullptr, (const float *)nullptr,
                           rvi, rvc, 0, (int64_t)0, (float *)nullptr);
    }
    RN_LAUNCH_CHECK(ctx);
    SweepArgs a{n, ray_idxs, stacked_views(ctx->p, features), P, P_inv, cc, nullptr, nullptr,
                nullptr, rvi, rvc, nullptr, S_voxel, nullptr, nullptr};
    launch_sweep<1, false>(ctx, a, true, st);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_mvcnn_voxel_space(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                         const float *P, const float *P_inv, const float *camera_center,
                         int32_t *rvi, int32_t *rvc, float *S_voxel, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, rvi, rvc, S_voxel));
    int rc = need_axes(ctx);
    if (rc) return rc;
    return prefix_api(ctx, n, ray_idxs, features, P, P_inv, camera_center, rvi, rvc, S_voxel,
                      S(stream));
}

int rn_mvcnn_voxel_space_depth(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs,
                               const float *features, const float *P, const float *P_inv,
                               const float *camera_center, int32_t *rvi, int32_t *rvc,
                               float *S_voxel, float *depth_map, void *stream) {
    if (!depth_map) return fail(ctx, RN_ERR_INVALID, "bad argument");
    int rc = rn_mvcnn_voxel_space(ctx, n, ray_idxs, features, P, P_inv, camera_center, rvi, rvc,
                                  S_voxel, stream);
    if (rc || n == 0) return rc;
    ProfScope prof(ctx, RN_K_DEPTH, n, S(stream));
    hipLaunchKernelGGL((k_argmax_depth<false>), dim3(ray_blocks(n)), dim3(BLOCK), 0, S(stream),
                       ctx->p, n, S_voxel, rvi, rvc, ctx->axes, camera_center, depth_map);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_fused_bp_sweep(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                      const float *P, const float *P_inv, const float *camera_center,
                      int32_t *rvi, int32_t *rvc, float *S_voxel, const float *acc_in,
                      const float *msgs_in, float *acc_out, float *msgs_out, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, rvi, rvc, S_voxel, acc_in,
                            msgs_in, acc_out, msgs_out));
    int rc = need_axes(ctx);
    if (rc) return rc;
    rc = prefix_api(ctx, n, ray_idxs, features, P, P_inv, camera_center, rvi, rvc, S_voxel,
                    S(stream));
    if (rc) return rc;
    return launch_bp<false, true>(ctx, n, S_voxel, rvi, rvc, acc_in, msgs_in, acc_out, msgs_out,
                                  S(stream));
}

int rn_fused_depth(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                   const float *P, const float *P_inv, const float *camera_center, int32_t *rvi,
                   int32_t *rvc, float *S_voxel, const float *acc, const float *msgs,
                   float *depth_map, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, features, P, P_inv, camera_center, rvi, rvc, S_voxel, acc,
                            msgs, depth_map));
    int rc = need_axes(ctx);
    if (rc) return rc;
    rc = prefix_api(ctx, n, ray_idxs, features, P, P_inv, camera_center, rvi, rvc, S_voxel,
                    S(stream));
    if (rc) return rc;
    // the reference overwrites S_voxel_space with the final distribution (raynet_fp.py:183-190)
    return launch_depth<false, true>(ctx, n, S_voxel, rvi, rvc, acc, msgs, camera_center, S_voxel,
                                     depth_map, S(stream));
}

// ------------------------------------------------------ resident-scene path
int rn_acc_copies(const rn_ctx *ctx) { return ctx ? 1 : 0; }

int rn_scatter_reset(rn_ctx *ctx) {
    if (!ctx) return RN_ERR_INVALID;
    ctx->box.reset();
    return RN_OK;
}

int rn_scatter_settled(const rn_ctx *ctx) {
    return ctx && ctx->box.settled() ? 1 : 0;
}

int64_t rn_slab_boxes_size(const rn_ctx *ctx, int64_t rows) {
    return ctx && rows >= 0 ? ((rows + WAVE - 1) / WAVE) * slab_box_count(ctx->p.M) * 2 : 0;
}

int rn_scene_bind_slab_boxes(rn_ctx *ctx, const int32_t *vox, int64_t rows, int32_t *boxes) {
    if (!ctx || rows < 0 || (boxes && !vox)) return fail(ctx, RN_ERR_INVALID, "bad argument");
    ctx->sb_vox = boxes ? vox : nullptr;
    ctx->sb_rows = boxes ? rows : 0;
    ctx->sb_boxes = reinterpret_cast<int2 *>(boxes);
    ctx->sb_valid_lo = ctx->sb_valid_hi = 0;
    return RN_OK;
}

int rn_scene_bind_scatter_items(rn_ctx *ctx, const int32_t *vox, int64_t rows, int32_t level,
                                const int32_t *items, int32_t count) {
    if (!ctx || rows < 0 || count < 0 || level < 0 || level > 1 || (items && (!vox || count < 1)))
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    // an item is `tile << 12 | first << 6 | count` in 32 bits: 19 bits of tile index
    if (items && (rows + (level == 0 ? 127 : 255)) / (level == 0 ? 128 : 256) > (int64_t(1) << 19))
        return fail(ctx, RN_ERR_INVALID, "rn_scene_bind_scatter_items: %lld rows are more than "
                    "2^19 tiles of level %d; use the tiles x split launch (no work list)",
                    (long long)rows, level);
    ctx->sc_vox = items ? vox : nullptr;
    ctx->sc_items = items;
    ctx->sc_rows = items ? rows : 0;
    ctx->sc_level = level;
    ctx->sc_count = items ? count : 0;
    return RN_OK;
}

int rn_scatter_state(const rn_ctx *ctx, int32_t *level, uint32_t *chunks, uint32_t *overflowed) {
    if (!ctx || !level || !chunks || !overflowed) return RN_ERR_INVALID;
    ctx->box.state(level, chunks, overflowed);
    return RN_OK;
}

int64_t rn_acc_size(const rn_ctx *ctx) { return ctx ? acc_floats(ctx) : 0; }

int rn_acc_to_grid(rn_ctx *ctx, const float *acc, float *grid_out, void *stream) {
    if (!ctx || !acc || !grid_out) return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int64_t G = (int64_t)ctx->p.gx * ctx->p.gy * ctx->p.gz;
    hipLaunchKernelGGL((k_acc_regrid<true>), dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream),
                       ctx->p, acc, grid_out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_stitch_rows(rn_ctx *ctx, int64_t n, const float *rows, const int32_t *index, float *out,
                   void *stream) {
    if (!ctx || n < 0 || (n && (!rows || !index || !out)) || ((uintptr_t)out & 15) ||
        ((uintptr_t)index & 15))
        return fail(ctx, RN_ERR_INVALID, "rn_stitch_rows: bad argument");
    if (n == 0) return RN_OK;
    // page-locked host memory: the kernel writes through its device-side address
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, out) == hipSuccess && at.type == hipMemoryTypeHost) {
        if (!at.devicePointer)
            return fail(ctx, RN_ERR_INVALID, "rn_stitch_rows: host memory that is not mapped");
        out = static_cast<float *>(at.devicePointer);
    } else {
        (void)hipGetLastError();       // (an unregistered pointer: reported by the launch)
    }
    // 64 workgroups keep a PCIe link busy (16: 3 % slower per step of an eight-rank shard); one
    // per CU only takes issue slots from the depth sweep this launch runs under (300: 1.5 %)
    int nb = fill_blocks((n + 3) / 4);
    if (nb > 64) nb = 64;
    hipLaunchKernelGGL(k_stitch_rows, dim3(nb), dim3(BLOCK), 0, S(stream), n,
                       rows, index, out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_acc_from_grid(rn_ctx *ctx, const float *grid, float *acc_out, void *stream) {
    if (!ctx || !grid || !acc_out) return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int64_t G = (int64_t)ctx->p.gx * ctx->p.gy * ctx->p.gz;
    hipLaunchKernelGGL((k_acc_regrid<false>), dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream),
                       ctx->p, grid, acc_out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_scene_prepare(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs,
                     const float *const *features_views_host, const float *P, const float *P_inv,
                     const float *camera_center, const int32_t *order, int32_t *vox, int32_t *rvc,
                     float *Sr, float *ray_segments, void *stream) {
    RN_OPEN(ctx, n, all_set(ray_idxs, features_views_host, P, P_inv, camera_center, vox, rvc, Sr));
    int rc = need_axes(ctx);
    if (rc) return rc;
    if (ctx->sb_boxes && vox >= ctx->sb_vox && vox < ctx->sb_vox + ctx->sb_rows * (int64_t)ctx->p.M)
        ctx->sb_valid_lo = ctx->sb_valid_hi = 0;      // this entry does not maintain slab boxes
    FeatureViews fv;
    for (int v = 0; v < MAX_VIEWS; v++) fv.v[v] = v < ctx->p.N ? features_views_host[v] : nullptr;
    for (int v = 0; v < ctx->p.N; v++)
        if (!fv.v[v]) return fail(ctx, RN_ERR_INVALID, "null feature map for view %d", v);
    {
        ProfScope prof(ctx, RN_K_TRAVERSE, n, S(stream));
        hipLaunchKernelGGL((k_traverse<true>), dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, S(stream),
                           ctx->p, n, ray_idxs, P_inv, camera_center, (const float *)nullptr,
                           (const float *)nullptr, vox, rvc, 0, (int64_t)0, ray_segments);
    }
    RN_LAUNCH_CHECK(ctx);
    SweepArgs a{n, ray_idxs, fv, P, P_inv, camera_center, nullptr, nullptr, nullptr, vox, rvc,
                nullptr, Sr, nullptr, nullptr};
    a.order = order;
    a.seg = ray_segments;
    launch_sweep<2, true>(ctx, a, true, S(stream));
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"

// rn_scene_prepare_all; with msgs_fold the plane sweep also writes BP iteration 0's messages
// (k_sweep_map MAPMODE 3, first_sweep_messages)
// The one occupancy of BP iteration 0 (the prior in every voxel, no messages), evaluated by the
// device's own arithmetic once per prior value and kept with the context.
static int first_occupancy(rn_ctx *ctx, float prior, hipStream_t st, float *out) {
    if (!ctx->have_first_occ || ctx->first_prior != prior) {
        hipLaunchKernelGGL(k_first_occupancy, dim3(1), dim3(1), 0, st, prior, ctx->scalar_dev);
        hipError_t e = hipMemcpyAsync(&ctx->first_occ, ctx->scalar_dev, sizeof(float),
                                      hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);      // (once per prior value)
        if (e != hipSuccess) return fail(ctx, RN_ERR_HIP, "first_occupancy: %s", hipGetErrorString(e));
        ctx->first_prior = prior;
        ctx->have_first_occ = true;
    }
    *out = ctx->first_occ;
    return RN_OK;
}

static int scene_prepare_all_impl(rn_ctx *ctx, int32_t n_images, int32_t n, int64_t rows_per_image,
                                  const int32_t *ray_idxs, const float *const *features_views,
                                  const float *cameras, const int32_t *order, int32_t *vox,
                                  int32_t *rvc, float *Sr, float *ray_segments, void *stream,
                                  float *msgs_fold, float prior, float *zero_fold = nullptr,
                                  int sweep_xcd_chunk = 0) {
    if (ctx && n == 0 && n_images >= 1) return RN_OK;   /* a rank without rays: pointers may be null */
    if (!ctx || n_images < 1 || n < 0 || rows_per_image < n || !ray_idxs || !features_views ||
        !cameras || !vox || !rvc || !Sr)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    int rc = need_axes(ctx);
    if (rc) return rc;
    const int N = ctx->p.N;
    const int cam_stride = 12 * N + 12 + 4;
    const size_t M = (size_t)ctx->p.M;
    float o_first = 0.0f;
    if (msgs_fold) {
        rc = first_occupancy(ctx, prior, S(stream), &o_first);
        if (rc) return rc;
    }
    // slab boxes for the scatter, when a table is bound to this list buffer (rows_per_image is
    // then a multiple of 64 by the binding's contract: checked)
    int2 *boxes = rows_per_image % WAVE == 0
                      ? slab_boxes_for(ctx, vox, (int64_t)n_images * rows_per_image, false) : nullptr;
    if (ctx->sb_boxes && vox >= ctx->sb_vox && vox < ctx->sb_vox + ctx->sb_rows * (int64_t)M) {
        if (boxes) {
            ctx->sb_valid_lo = (vox - ctx->sb_vox) / (int64_t)M;
            ctx->sb_valid_hi = ctx->sb_valid_lo + (int64_t)n_images * rows_per_image;
        } else {
            ctx->sb_valid_lo = ctx->sb_valid_hi = 0;
        }
    }
    // traverse + sweep of images [g0, g0 + ng); the traversal on `trav_st`, the sweep on `st`
    auto traverse = [&](int g0, int ng, hipStream_t trav_st) {
        const float *cam = cameras + (size_t)g0 * cam_stride;
        const size_t row0 = (size_t)g0 * rows_per_image;
        ProfScope prof(ctx, RN_K_TRAVERSE, n * ng, trav_st);
        hipLaunchKernelGGL((k_traverse<true>), dim3((n + WAVE - 1) / WAVE, ng), dim3(WAVE), 0,
                           trav_st, ctx->p, n, ray_idxs, cam + 12 * N, cam + 12 * N + 12,
                           (const float *)nullptr, (const float *)nullptr, vox + row0 * M,
                           rvc + row0, cam_stride, rows_per_image,
                           ray_segments ? ray_segments + row0 * 8 : nullptr,
                           boxes ? boxes + (row0 / WAVE) * slab_box_count(ctx->p.M) : nullptr);
    };
    auto sweep = [&](int g0, int ng, hipStream_t st) {
        const float *cam = cameras + (size_t)g0 * cam_stride;
        const size_t row0 = (size_t)g0 * rows_per_image;
        SweepArgs a{n, ray_idxs, FeatureViews{}, cam, cam + 12 * N, cam + 12 * N + 12, nullptr,
                    nullptr, nullptr, vox + row0 * M, rvc + row0, nullptr, Sr + row0 * M, nullptr,
                    nullptr};
        a.order = order;
        a.fv_table = features_views + (size_t)g0 * N;
        a.cam_stride = cam_stride;
        a.rows_per_image = rows_per_image;
        a.n_images = ng;
        a.seg = ray_segments ? ray_segments + row0 * 8 : nullptr;
        a.xcd_chunk = sweep_xcd_chunk / SWEEP_WAVES;
        if (msgs_fold) {
            a.msgs_out = msgs_fold + row0 * M;
            a.prior = o_first;
            a.zero = g0 == 0 ? zero_fold : nullptr;      // (once per pass)
            launch_sweep<3, true>(ctx, a, true, st);
        } else {
            launch_sweep<2, true>(ctx, a, true, st);
        }
    };
    const bool split = ctx->overlap == 1 || (ctx->overlap == 2 && ctx->box.level == 1);
    const int gA = split && n_images >= 2 && (int64_t)n * n_images >= 65536
                       ? (n_images + 1) / 2 : n_images;
    if (gA < n_images) {
        // the thread-per-ray traversal (a chain of dependent fp32 additions per ray, few waves
        // per CU) of the second half of the images hides under the plane sweep of the first
        RN_HIP(ctx, hipEventRecord(ctx->ev_fork, S(stream)));
        RN_HIP(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
        traverse(0, gA, S(stream));
        RN_LAUNCH_CHECK(ctx);
        traverse(gA, n_images - gA, ctx->aux);
        RN_LAUNCH_CHECK(ctx);
        RN_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
        sweep(0, gA, S(stream));
        RN_LAUNCH_CHECK(ctx);
        RN_HIP(ctx, hipStreamWaitEvent(S(stream), ctx->ev_join, 0));
        sweep(gA, n_images - gA, S(stream));
        RN_LAUNCH_CHECK(ctx);
    } else {
        traverse(0, n_images, S(stream));
        RN_LAUNCH_CHECK(ctx);
        sweep(0, n_images, S(stream));
        RN_LAUNCH_CHECK(ctx);
    }
    return RN_OK;
}

extern "C" {

int rn_scene_prepare_all(rn_ctx *ctx, int32_t n_images, int32_t n, int64_t rows_per_image,
                         const int32_t *ray_idxs, const float *const *features_views,
                         const float *cameras, const int32_t *order, int32_t *vox, int32_t *rvc,
                         float *Sr, float *ray_segments, void *stream) {
    return scene_prepare_all_impl(ctx, n_images, n, rows_per_image, ray_idxs, features_views, cameras,
                                  order, vox, rvc, Sr, ray_segments, stream, nullptr, 0.0f);
}

int rn_scene_count_voxels(rn_ctx *ctx, int32_t n_images, int32_t n, const int32_t *ray_idxs,
                          const float *cameras, int32_t *rvc, void *stream) {
    if (ctx && n == 0 && n_images >= 1) return RN_OK;   /* empty launch: pointers may be null */
    if (!ctx || n_images < 1 || n < 0 || !ray_idxs || !cameras || !rvc)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int N = ctx->p.N;
    const int cam_stride = 12 * N + 12 + 4;
    ProfScope prof(ctx, RN_K_TRAVERSE, n * n_images, S(stream));
    hipLaunchKernelGGL((k_traverse<true>), dim3((n + WAVE - 1) / WAVE, n_images), dim3(WAVE), 0,
                       S(stream), ctx->p, n, ray_idxs, cameras + 12 * N, cameras + 12 * N + 12,
                       (const float *)nullptr, (const float *)nullptr, (int32_t *)nullptr, rvc,
                       cam_stride, (int64_t)n, (float *)nullptr);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_scene_bp_sweep(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                      const int32_t *rvc, const float *acc_in, float *msgs, float *acc_part,
                      int32_t first_sweep, int32_t row_layout, void *stream) {
    RN_OPEN(ctx, n, all_set(Sr, vox, rvc, acc_in, msgs, acc_part));
    return launch_bp<true, false>(ctx, n, Sr, vox, rvc, acc_in,
                                  (first_sweep & RN_SWEEP_ZERO_MSGS) ? nullptr : msgs, acc_part,
                                  msgs, S(stream), row_layout == RN_ROWS_PATCHES, false,
                                  uniform_mode((first_sweep & RN_SWEEP_UNIFORM_ACC) != 0));
}

int rn_scene_bp_sweep_fixed(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                            const int32_t *rvc, const float *acc_in, float *msgs,
                            int64_t *acc_part_fixed, int32_t first_sweep, int32_t row_layout,
                            void *stream) {
    RN_OPEN(ctx, n, all_set(Sr, vox, rvc, acc_in, msgs, acc_part_fixed));
    return launch_bp<true, false>(ctx, n, Sr, vox, rvc, acc_in,
                                  (first_sweep & RN_SWEEP_ZERO_MSGS) ? nullptr : msgs,
                                  acc_part_fixed, msgs, S(stream), row_layout == RN_ROWS_PATCHES,
                                  true, uniform_mode((first_sweep & RN_SWEEP_UNIFORM_ACC) != 0));
}

int rn_acc_combine_fixed(rn_ctx *ctx, int64_t *acc_part_fixed, float prior, float *acc_out,
                         void *stream) {
    if (!ctx || !acc_part_fixed || !acc_out) return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int64_t G = acc_floats(ctx);
    ProfScope prof(ctx, RN_K_ACC, 0, S(stream));
    hipLaunchKernelGGL(k_acc_combine_fixed, dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream),
                       reinterpret_cast<unsigned long long *>(acc_part_fixed), G, prior, acc_out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_acc_combine_fixed_range(rn_ctx *ctx, int64_t *acc_part_fixed, int64_t count, float prior,
                               float *acc_out, void *stream) {
    if (!ctx || !acc_part_fixed || !acc_out || count < 0)
        return fail(ctx, RN_ERR_INVALID, "bad argument");
    if (count == 0) return RN_OK;
    ProfScope prof(ctx, RN_K_ACC, 0, S(stream));
    hipLaunchKernelGGL(k_acc_combine_fixed, dim3(fill_blocks(count)), dim3(BLOCK), 0, S(stream),
                       reinterpret_cast<unsigned long long *>(acc_part_fixed), count, prior, acc_out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_acc_combine(rn_ctx *ctx, float *acc_part, float prior, float *acc_out, void *stream) {
    if (!ctx || !acc_part || !acc_out) return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int64_t G = acc_floats(ctx);
    ProfScope prof(ctx, RN_K_ACC, 0, S(stream));
    hipLaunchKernelGGL(k_acc_combine, dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream), acc_part,
                       1, G, prior, acc_out, 1);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_acc_reduce_local(rn_ctx *ctx, float *acc_part, float *acc_out, void *stream) {
    if (!ctx || !acc_part || !acc_out) return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int64_t G = acc_floats(ctx);
    ProfScope prof(ctx, RN_K_ACC, 0, S(stream));
    hipLaunchKernelGGL(k_acc_combine, dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream), acc_part,
                       1, G, 0.0f, acc_out, 0);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_acc_add_prior(rn_ctx *ctx, float *acc, float prior, void *stream) {
    if (!ctx || !acc) return fail(ctx, RN_ERR_INVALID, "bad argument");
    const int64_t G = acc_floats(ctx);
    hipLaunchKernelGGL(k_add_scalar, dim3(fill_blocks(G)), dim3(BLOCK), 0, S(stream), acc, G,
                       prior);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_scene_depth(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                   const int32_t *rvc, const float *acc, const float *msgs,
                   const float *camera_center, int32_t rays_per_center, float *S_new,
                   float *depth_map, void *stream) {
    RN_OPEN(ctx, n, all_set(Sr, vox, rvc, acc, msgs) && (S_new || depth_map) &&
                        (!depth_map || camera_center));
    int rc = need_axes(ctx);
    if (rc) return rc;
    if (rays_per_center < 0) return fail(ctx, RN_ERR_INVALID, "bad argument");
    return launch_depth<true, false>(ctx, n, Sr, vox, rvc, acc, msgs, camera_center, S_new,
                                     depth_map, S(stream), rays_per_center);
}

int rn_scene_depth_stats(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                         const int32_t *rvc, const float *acc, const float *msgs,
                         const float *camera_center, int32_t rays_per_center, float *S_new,
                         float *depth_map, float *stats, int64_t stats_stride, void *stream) {
    // (before the empty-launch shortcut: asking for statistics without a place for them is an
    // error at any n, never a plain depth sweep)
    if (ctx && !stats) return fail(ctx, RN_ERR_INVALID, "rn_scene_depth_stats: stats is required");
    RN_OPEN(ctx, n, all_set(Sr, vox, rvc, acc, msgs, depth_map, camera_center));
    if (rays_per_center < 0 || stats_stride < n)
        return fail(ctx, RN_ERR_INVALID, "rn_scene_depth_stats: bad rays_per_center or stats_stride");
    int rc = need_axes(ctx);
    if (rc) return rc;
    DepthStats out;
    out.planes = stats;
    out.stride = stats_stride;
    return launch_depth<true, false>(ctx, n, Sr, vox, rvc, acc, msgs, camera_center, S_new,
                                     depth_map, S(stream), rays_per_center, AccMode(), 4,
                                     DepthDest(), out);
}

int rn_scene_run(rn_ctx *ctx, const rn_scene_plan *pl, int32_t phases, int32_t iteration,
                 int32_t image, void *stream) {
    if (!ctx || !pl || pl->n_images < 1 || pl->n < 0 || pl->rows_per_image < pl->n ||
        pl->rows_per_image % 256 || iteration < 0 ||
        (!(phases & RN_RUN_DEPTH_RANGE) && image >= pl->n_images) ||
        (!pl->ray_idxs && pl->n) || !pl->features_views || !pl->cameras || !pl->vox || !pl->rvc || !pl->Sr || !pl->msgs ||
        !pl->acc[0] || !pl->acc[1] || !pl->depth ||
        (pl->depth_image && pl->depth_image_stride < 1) ||
        (pl->stats_image && (!pl->depth_image ||
                             pl->stats_image_stride < pl->n_images * pl->depth_image_stride)) ||
        pl->sweep_xcd_chunk < 0 ||
        pl->sweep_xcd_chunk % 4 ||
        (phases & ~(RN_RUN_PREPARE | RN_RUN_SWEEP | RN_RUN_COMBINE | RN_RUN_DEPTH | RN_RUN_DEPTH_RANGE)) ||
        ((phases & RN_RUN_DEPTH_RANGE) &&
         (image < 0 || (image >> 16) < 1 || (image & 0xffff) + (image >> 16) > pl->n_images ||
          (phases & RN_RUN_DEPTH))))
        return fail(ctx, RN_ERR_INVALID, "rn_scene_run: bad plan or phase");
    int rc = need_axes(ctx);
    if (rc) return rc;
    const bool fixed = pl->acc_fixed != nullptr;
    const int64_t rows = (int64_t)pl->n_images * pl->rows_per_image;
    if (rows > 0x7fffffff) return fail(ctx, RN_ERR_INVALID, "rn_scene_run: too many rows");
    hipStream_t st = S(stream);
    const int64_t G = acc_floats(ctx);
    bool folded = false;
    if (phases & RN_RUN_PREPARE) {
        if (fixed) RN_HIP(ctx, hipMemsetAsync(pl->acc_fixed, 0, sizeof(int64_t) * G, st));
        // K1 prefix and BP iteration 0 requested together: the plane sweep writes the first
        // messages itself (one occupancy for every voxel, nothing to gather) while the column
        // is still in LDS; SWEEP(0) below is then the scatter alone
        folded = (phases & RN_RUN_SWEEP) && iteration == 0 && fold_fits(ctx->p);
        if (pl->n > 0)
            rc = scene_prepare_all_impl(ctx, pl->n_images, pl->n, pl->rows_per_image, pl->ray_idxs,
                                        pl->features_views, pl->cameras, pl->order, pl->vox,
                                        pl->rvc, pl->Sr, pl->ray_segments, stream,
                                        folded ? pl->msgs : nullptr, pl->prior,
                                        folded && !fixed ? pl->acc[0] : nullptr,
                                        pl->sweep_xcd_chunk);
        if (rc) return rc;
    }
    if (pl->n == 0) {
        // a rank without rays (tiny images, many ranks) still takes part in the exchange: its
        // partial sums are all zero
        if ((phases & RN_RUN_SWEEP) && !fixed)
            RN_HIP(ctx, hipMemsetAsync(pl->acc[iteration & 1], 0, sizeof(float) * G, st));
        if ((phases & RN_RUN_COMBINE) && fixed)
            return rn_acc_combine_fixed(ctx, pl->acc_fixed, pl->prior, pl->acc[iteration & 1], stream);
        return RN_OK;
    }
    if (phases & RN_RUN_SWEEP) {
        AccMode am;
        am.uniform = iteration == 0;        // the prior everywhere, no messages yet
        am.biased = !fixed || iteration == 0;
        am.bias = pl->prior;
        am.zero = fixed ? nullptr : pl->acc[iteration & 1];
        rc = launch_bp<true, false>(ctx, (int)rows, pl->Sr, pl->vox, pl->rvc,
                                    pl->acc[(iteration + 1) & 1], iteration == 0 ? nullptr : pl->msgs,
                                    fixed ? (void *)pl->acc_fixed : (void *)pl->acc[iteration & 1],
                                    pl->msgs, st, pl->row_layout == RN_ROWS_PATCHES, fixed, am,
                                    folded);
        if (rc) return rc;
    }
    if ((phases & RN_RUN_COMBINE) && fixed) {
        rc = rn_acc_combine_fixed(ctx, pl->acc_fixed, pl->prior, pl->acc[iteration & 1], stream);
        if (rc) return rc;
    }
    if (phases & (RN_RUN_DEPTH | RN_RUN_DEPTH_RANGE)) {
        AccMode am;
        am.biased = !fixed;
        am.bias = pl->prior;
        const float *acc = pl->acc[(iteration + 1) & 1];
        const int cam_stride = 12 * ctx->p.N + 12 + 4;
        const float *cc = pl->cameras + 12 * ctx->p.N + 12;
        const size_t M = (size_t)ctx->p.M;
        // depth_image: the maps leave in pixel order (no reordering pass behind the sweep)
        DepthDest dest;
        if (pl->depth_image) {
            dest.pixel_of_row = pl->ray_idxs;
            dest.rows = pl->n;
            dest.image_stride = pl->depth_image_stride;
        }
        auto out = [&](int first) {
            return pl->depth_image ? pl->depth_image + (size_t)first * pl->depth_image_stride
                                   : pl->depth + (size_t)first * pl->rows_per_image;
        };
        // the statistics go where the depths go: pixel order next to depth_image, else row order
        auto stats = [&](int first) {
            DepthStats s;
            if (pl->depth_image ? pl->stats_image != nullptr : pl->stats != nullptr) {
                s.planes = pl->depth_image ? pl->stats_image + (size_t)first * pl->depth_image_stride
                                           : pl->stats + (size_t)first * pl->rows_per_image;
                s.stride = pl->depth_image ? pl->stats_image_stride : rows;
            }
            return s;
        };
        if (image < 0)
            return launch_depth<true, false>(ctx, (int)rows, pl->Sr, pl->vox, pl->rvc, acc, pl->msgs, cc,
                                             nullptr, out(0), st, (int)pl->rows_per_image, am,
                                             cam_stride, dest, stats(0));
        if (phases & RN_RUN_DEPTH_RANGE) {
            const int first = image & 0xffff, count = image >> 16;
            const size_t r0 = (size_t)first * pl->rows_per_image;
            return launch_depth<true, false>(ctx, (int)(count * pl->rows_per_image), pl->Sr + r0 * M,
                                             pl->vox + r0 * M, pl->rvc + r0, acc, pl->msgs + r0 * M,
                                             cc + (size_t)first * cam_stride, nullptr, out(first),
                                             st, (int)pl->rows_per_image, am, cam_stride, dest,
                                             stats(first));
        }
        const size_t row0 = (size_t)image * pl->rows_per_image;
        // (one image: a single group of rows_per_image >= n rows)
        return launch_depth<true, false>(ctx, pl->n, pl->Sr + row0 * M, pl->vox + row0 * M,
                                         pl->rvc + row0, acc, pl->msgs + row0 * M,
                                         cc + (size_t)image * cam_stride, nullptr, out(image),
                                         st, 0, am, 4, dest, stats(image));
    }
    return RN_OK;
}

int rn_prof_begin(rn_ctx *ctx, int32_t capacity) {
    if (!ctx || capacity < 1) return fail(ctx, RN_ERR_INVALID, "bad argument");
    if (capacity > ctx->prof_cap) {
        hipEvent_t *ev = new hipEvent_t[2 * capacity];
        for (int i = 0; i < 2 * ctx->prof_cap; i++) ev[i] = ctx->prof_ev[i];
        for (int i = 2 * ctx->prof_cap; i < 2 * capacity; i++) RN_HIP(ctx, hipEventCreate(&ev[i]));
        delete[] ctx->prof_ev;
        delete[] ctx->prof_id;
        delete[] ctx->prof_rays;
        ctx->prof_ev = ev;
        ctx->prof_id = new int32_t[capacity];
        ctx->prof_rays = new int32_t[capacity];
        ctx->prof_cap = capacity;
    }
    ctx->prof_n = 0;
    ctx->prof_on = true;
    return RN_OK;
}

int rn_prof_select(rn_ctx *ctx, uint32_t kernel_mask) {
    if (!ctx) return RN_ERR_INVALID;
    ctx->prof_mask = kernel_mask;
    return RN_OK;
}

int rn_prof_end(rn_ctx *ctx, int32_t *count, int32_t *kernel_ids_host, int32_t *n_rays_host,
                float *ms_host) {
    if (!ctx || !count) return fail(ctx, RN_ERR_INVALID, "bad argument");
    ctx->prof_on = false;
    const int n = ctx->prof_n;
    for (int i = 0; i < n; i++) {
        RN_HIP(ctx, hipEventSynchronize(ctx->prof_ev[2 * i + 1]));
        float ms = 0.0f;
        RN_HIP(ctx, hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
        if (ms_host) ms_host[i] = ms;
        if (kernel_ids_host) kernel_ids_host[i] = ctx->prof_id[i];
        if (n_rays_host) n_rays_host[i] = ctx->prof_rays[i];
    }
    *count = n;
    return RN_OK;
}

int rn_selftest_arith(rn_ctx *ctx, int32_t n, const float *a, float *out, void *stream) {
    RN_OPEN(ctx, n, all_set(a, out));
    hipLaunchKernelGGL(k_selftest_arith, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, a, out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_selftest_quotient(rn_ctx *ctx, int32_t n, const float *x, const float *d, float *out,
                         void *stream) {
    RN_OPEN(ctx, n, all_set(x, d, out));
    hipLaunchKernelGGL(k_selftest_quotient, dim3(thread_blocks(n)), dim3(BLOCK), 0, S(stream), n, x,
                       d, out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_selftest_feature_offsets(rn_ctx *ctx, int32_t n, const float *P, const float *ray_start,
                                const float *ray_end, int32_t *out, void *stream) {
    RN_OPEN(ctx, n, all_set(P, ray_start, ray_end, out));
    hipLaunchKernelGGL(k_selftest_offsets, dim3(ray_blocks(n)), dim3(BLOCK), 0, S(stream), ctx->p, n,
                       P, ray_start, ray_end, out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_selftest_mapping(rn_ctx *ctx, int32_t n, const float *a, const float *b, const float *t,
                        float *out, void *stream) {
    RN_OPEN(ctx, n, all_set(a, b, t, out));
    hipLaunchKernelGGL(k_selftest_mapping, dim3(thread_blocks(n)), dim3(BLOCK),
                       sizeof(float) * (ctx->p.D + 1), S(stream), ctx->p, n, a, b, t, out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

int rn_prof_offsets(rn_ctx *ctx, float *start_ms_host) {
    if (!ctx || !start_ms_host) return fail(ctx, RN_ERR_INVALID, "bad argument");
    for (int i = 0; i < ctx->prof_n; i++)
        RN_HIP(ctx, hipEventElapsedTime(start_ms_host + i, ctx->prof_ev[0], ctx->prof_ev[2 * i]));
    return RN_OK;
}


int rn_timer_start(rn_ctx *ctx, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    RN_HIP(ctx, hipEventRecord(ctx->ev0, S(stream)));
    return RN_OK;
}

int rn_timer_stop(rn_ctx *ctx, void *stream, float *ms_out) {
    if (!ctx || !ms_out) return RN_ERR_INVALID;
    RN_HIP(ctx, hipEventRecord(ctx->ev1, S(stream)));
    RN_HIP(ctx, hipEventSynchronize(ctx->ev1));
    RN_HIP(ctx, hipEventElapsedTime(ms_out, ctx->ev0, ctx->ev1));
    return RN_OK;
}

}  // extern "C"

// training (differentiable) entry points, SURVEY.md 8f row 2
#include "raynet_train.inl"

// depth maps -> point cloud -> accuracy / completeness, SURVEY.md 8f row 3
#include "raynet_eval.inl"

// ground-truth depth from scene meshes (BVH ray casting)
#include "raynet_mesh.inl"

// point-cloud filters: VoxelMask and the exact parallel ReduceDensity
#include "raynet_filters.inl"

// ground-truth depth of a point cloud: every view's z-buffer in one pass
#include "raynet_cloud.inl"

// training batches of rays from many reference views
#include "raynet_batch.inl"

// the occupancy volume: belief grid of an accumulator, rendered along rays
#include "raynet_volume.inl"

// what the surface looks like: vertex normals, colours from the scene's images (DESIGN.md
// section 20)
#include "raynet_appearance.inl"

// depth maps fused into a truncated signed distance volume
#include "raynet_fusion.inl"

// what the other views say about a point: seen, agreeing and violated masks
#include "raynet_consistency.inl"

// which views see a point, the points every pair of views shares, a covering set's gains: ballots,
// LDS counters and integer atomics
#include "raynet_overlap.inl"

// the connected components of a surface mesh: a lock-free union-find
#include "raynet_components.inl"

// Taubin smoothing of a surface mesh: a gather over the corner table
#include "raynet_smooth.inl"

// the grid-level exclusive scan of 64-bit words, in front of its two users
#include "raynet_scan.inl"

// vertex clustering of a surface mesh on a uniform grid: integer atomics and the scan (DESIGN.md
// section 24)
#include "raynet_simplify.inl"

// quadric-error placement of the clustered vertices: the planes of the faces summed per cluster
// in fixed point, a 3 x 3 solve per vertex
#include "raynet_quadric.inl"

// the small holes of a surface mesh capped: the union-find over the boundary half-edges, the
// corner table and the scan
#include "raynet_holes.inl"

// a surface mesh seen from cameras: face, depth, barycentrics, colours and normals per pixel over
// raynet_mesh.inl's BVH
#include "raynet_render.inl"

// the photographs baked into a texture atlas of a surface mesh, and the lookup behind a render
// 
#include "raynet_texture.inl"

// the surface of a belief grid: marching tetrahedra and the scan
#include "raynet_isosurface.inl"

