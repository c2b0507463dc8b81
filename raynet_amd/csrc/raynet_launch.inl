// raynet_launch.inl -- host side of raynet_hip.hip: the context, and the launchers that turn
// run-time shapes into kernel instantiations.  Included after the kernels, before the C ABI.

struct rn_ctx {
    rn_config cfg = {};
    Params p = {};
    float *axes = nullptr;    // device, gx+gy+gz
    bool have_axes = false;
    int scatter_mode = -1;    // rn_options: -1 by row layout (default), 0 slab, 2 LDS box
    int generic_sweep = 0;    // rn_options: reference-order plane sweep even for F = 32
    int sweep_rpw = 0;        // rn_options.sweep_rays_per_wave: 0 by D, 1 one ray per wavefront
    // LDS-box scatter: the tile shape in use (launch_bp), the device counters {chunks, overflowed
    // chunks} it is chosen by and their pinned host mirror (an asynchronous copy, it may lag a launch)
    BoxPolicy box;
    unsigned *box_stats = nullptr, *box_stats_host = nullptr;
    // occupancy_to_ray(prior, 0) as the device evaluates it, for the prior it was last asked for
    float first_prior = 0.0f, first_occ = 0.0f;
    bool have_first_occ = false;
    float *scalar_dev = nullptr;      // 4 bytes of device scratch owned by the context
    // rn_batch_rays / rn_batch_patches: "an index was out of range" (device word, pinned mirror),
    // allocated by the first such call
    int32_t *batch_bad = nullptr, *batch_bad_host = nullptr;
    // sample_in_range's ray segments between k_range_segments and the plane sweep: [2][rays][3]
    float *range_seg = nullptr;
    size_t range_seg_rays = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // slab boxes (rn_scene_bind_slab_boxes): table, the list buffer it describes, and the row
    // range rn_scene_prepare_all last filled
    const int32_t *sb_vox = nullptr;
    int64_t sb_rows = 0, sb_valid_lo = 0, sb_valid_hi = 0;
    int2 *sb_boxes = nullptr;
    // work list of the box scatter (rn_scene_bind_scatter_items): the row range and tile level it
    // was built for
    const int32_t *sc_vox = nullptr, *sc_items = nullptr;
    int64_t sc_rows = 0;
    int sc_level = 0, sc_count = 0;
    // second stream of the resident-scene launchers (RAYNET_HIP_OVERLAP=0 / 1, default: by
    // the scatter's tile level): the accumulator scatter of one half of a launch's rows runs
    // next to the BP sweep of the other half, the traversal of half of the images next to the
    // plane sweep of the rest.  Measured (profiles/r02_exp_overlap.txt): config 2 8.72 ->
    // 8.84 ms/step (either kernel alone already keeps the VALUs of every CU busy), config 4
    // 44.3 -> 42.5 (its scatter waits on L2 atomics at 3.9 hits per voxel) -- and config 4 is
    // where the adaptive scatter has stepped to its second tile shape, so that is the switch
    int overlap = 2;          // 0 off, 1 on, 2 (default) when the scatter runs at tile level >= 1
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // per-launch profiling (rn_prof_begin / rn_prof_end)
    bool prof_on = false;
    uint32_t prof_mask = ~0u;     // which rn_kernel_id families are bracketed (rn_prof_select)
    int prof_cap = 0, prof_n = 0;
    hipEvent_t *prof_ev = nullptr;    // 2 * prof_cap
    int32_t *prof_id = nullptr, *prof_rays = nullptr;
    // kernels this context has opted in to more than 64 KB of dynamic LDS, and how much
    // (lds_opt_in); a failed opt-in is reported by the launch check
    std::vector<std::pair<const void *, size_t>> lds_granted;
    hipError_t lds_optin_error = hipSuccess;
    size_t lds_optin_bytes = 0;
    char err[512] = "";
};

// Brackets one kernel launch with two events on its stream when profiling is on.
struct ProfScope {
    rn_ctx *c;
    hipStream_t st;
    int slot;
    ProfScope(rn_ctx *ctx, int id, int n_rays, hipStream_t s) : c(ctx), st(s), slot(-1) {
        if (c->prof_on && ((c->prof_mask >> id) & 1u) && c->prof_n < c->prof_cap) {
            slot = c->prof_n++;
            c->prof_id[slot] = id;
            c->prof_rays[slot] = n_rays;
            (void)hipEventRecord(c->prof_ev[2 * slot], st);
        }
    }
    ~ProfScope() {
        if (slot >= 0) (void)hipEventRecord(c->prof_ev[2 * slot + 1], st);
    }
};

namespace {

int fail(rn_ctx *ctx, int code, const char *fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define RN_HIP(ctx, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(ctx, RN_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define RN_LAUNCH_CHECK(ctx)                                                           \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if ((ctx)->lds_optin_error != hipSuccess) {                                    \
            const hipError_t o_ = (ctx)->lds_optin_error;                              \
            (ctx)->lds_optin_error = hipSuccess;                                       \
            return fail(ctx, RN_ERR_HIP, "the plane sweep's opt-in to %zu bytes of LDS "  \
                        "(hipFuncSetAttribute) failed: %s; its launch: %s",            \
                        (ctx)->lds_optin_bytes, hipGetErrorString(o_), hipGetErrorString(e_)); \
        }                                                                              \
        if (e_ != hipSuccess)                                                          \
            return fail(ctx, RN_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e_)); \
    } while (0)

// The opening of an entry over n rays: an empty launch is RN_OK (its pointers may be null),
// anything else needs a context, n > 0 and `args_ok` (usually all_set(...) of its pointers).
template <class... P>
inline bool all_set(const P *...ptrs) { return (... && (ptrs != nullptr)); }
#define RN_OPEN(ctx, n, args_ok)                                                       \
    do {                                                                               \
        if ((ctx) && (n) == 0) return RN_OK;                                           \
        if (!(ctx) || (n) < 0 || !(args_ok)) return fail(ctx, RN_ERR_INVALID, "bad argument"); \
    } while (0)

inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }
inline int ray_blocks(int n) { return (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK; }
inline int ray_blocks_mrf(int n) { return (n + RAY_BLOCK / WAVE - 1) / (RAY_BLOCK / WAVE); }
inline int thread_blocks(int n) { return (n + BLOCK - 1) / BLOCK; }
inline int fill_blocks(int64_t n) {
    int64_t b = (n + BLOCK - 1) / BLOCK;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
inline int sweep_blocks(int n) { return (n + SWEEP_WAVES - 1) / SWEEP_WAVES; }
// rays a wavefront of the cooperative sweep takes (k_sweep_map_packed for 2 / 4)
inline int sweep_rays_per_wave(const rn_ctx *ctx) {
    if (ctx->sweep_rpw == 1) return 1;
    return ctx->p.D <= 16 ? 4 : ctx->p.D <= 32 ? 2 : 1;
}

// Dynamic LDS of a plane-sweep workgroup: the axis tables, the plane positions and per wavefront
// the columns of its `rpw` rays (k_sweep_map_packed: D <= 64 / rpw) and `rows` rows of M.
constexpr size_t sweep_lds_bytes(int axes, int D, int M, int rows, int rpw) {
    return sizeof(float) * ((size_t)((axes + 3) & ~3) + (size_t)((D + 4) & ~3) +
                            (size_t)SWEEP_WAVES * ((size_t)rpw * D + (size_t)rows * M));
}
inline size_t sweep_lds(const Params &p, int rows = 1, int rpw = 1) {
    return sweep_lds_bytes(p.gx + p.gy + p.gz, p.D, p.M, rows, rpw);
}
// what rn_create admits; no shape within these limits asks for more LDS than a CU of gfx950 has
// (110,608 bytes for one row set, 143,376 for the fold's three)
constexpr int MAX_M = 1024, MAX_D = 4096, MAX_GRID_AXIS = 1024;
constexpr size_t LDS_PER_CU = 160 * 1024;
static_assert(sweep_lds_bytes(3 * MAX_GRID_AXIS, MAX_D, MAX_M, 3, 1) <= LDS_PER_CU &&
              sweep_lds_bytes(3 * MAX_GRID_AXIS, 32, MAX_M, 3, 2) <= LDS_PER_CU &&
              sweep_lds_bytes(3 * MAX_GRID_AXIS, 16, MAX_M, 3, 4) <= LDS_PER_CU,
              "a plane sweep rn_create admits must fit the LDS of one CU");
// LDS a workgroup of the plane sweep may take and still leave room for SWEEP_MIN_WAVES
// wavefronts per SIMD (4 per workgroup, 160 KB per CU)
inline bool fold_fits(const Params &p) {
    return sweep_lds(p, 3) <= LDS_PER_CU / ((SWEEP_MIN_WAVES * 4 + SWEEP_WAVES - 1) / SWEEP_WAVES);
}

// floats of one resident (bricked) accumulator: every axis padded to a multiple of 4
inline int64_t acc_floats(const rn_ctx *ctx) {
    return (int64_t)((ctx->p.gx + 3) / 4) * ctx->p.nby * ctx->p.nbz * 64;
}

FeatureViews stacked_views(const Params &p, const float *features) {
    FeatureViews fv;
    const size_t dim = (size_t)p.Hf * p.Wf * p.F;
    for (int v = 0; v < MAX_VIEWS; v++) fv.v[v] = v < p.N ? features + dim * v : nullptr;
    return fv;
}

// ---- run-time values -> template arguments: f gets a std::integral_constant
template <int V> using int_c = std::integral_constant<int, V>;
// f(int_c<V>) for the V of the list that equals v; false when there is none
template <int... Vs, class F>
inline bool with_value(int v, F &&f) {
    return (... || (v == Vs && (f(int_c<Vs>{}), true)));
}
template <class F>
inline void with_bool(bool flag, F &&f) {
    if (flag) f(std::true_type{}); else f(std::false_type{});
}
// chunks of 64 list entries a body of k_bp / k_depth is compiled for: f(int_c<NCH>) for the
// smallest NCH >= nch (the last one holds the longest row rn_create admits)
constexpr int CHUNKS[] = {2, 4, 6, 8, 12, 16};
static_assert(CHUNKS[std::size(CHUNKS) - 1] * WAVE >= MAX_M, "no k_bp / k_depth body for the longest row");
template <size_t I = 0, class F>
inline void with_chunks(int nch, F &&f) {
    if constexpr (I + 1 < std::size(CHUNKS)) {
        if (nch > CHUNKS[I]) return with_chunks<I + 1>(nch, f);
    }
    f(int_c<CHUNKS[I]>{});
}

// gfx950 has 160 KB of LDS per CU; beyond 64 KB a kernel has to say so, per device -- so once per
// context, kernel and size.  A refusal is kept for the launch check to report.
inline void lds_opt_in(rn_ctx *ctx, const void *kernel, size_t lds) {
    if (lds <= 64 * 1024) return;
    auto g = ctx->lds_granted.begin();
    while (g != ctx->lds_granted.end() && g->first != kernel) ++g;
    if (g != ctx->lds_granted.end() && lds <= g->second) return;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctx->lds_optin_error = e;
        ctx->lds_optin_bytes = lds;
    } else if (g != ctx->lds_granted.end()) {
        g->second = lds;
    } else {
        ctx->lds_granted.emplace_back(kernel, lds);
    }
}

struct SweepArgs {
    int n;
    const int32_t *ray_idxs;
    FeatureViews fv;
    const float *P, *P_inv, *cc, *starts, *ends, *S_in;
    const int32_t *vox, *rvc;
    float *S_planes, *S_voxel, *depth_from_planes, *points;
    const int32_t *order = nullptr;
    // scene-wide launch (rn_scene_prepare_all): one grid row per reference image
    const float *const *fv_table = nullptr;
    int cam_stride = 0;
    int64_t rows_per_image = 0;
    int n_images = 1;
    const float *seg = nullptr;     // [rows][8]: ray segments written by k_traverse
    float *msgs_out = nullptr;      // MAPMODE 3: BP iteration 0's messages
    float prior = 0.0f;             // MAPMODE 3: occupancy_to_ray(prior, 0), see first_occupancy()
    float *zero = nullptr;          // MAPMODE 3: cleared on the side (rn_acc_size floats)
    int xcd_chunk = 0;              // workgroups per XCD group (0: XCD_CHUNK_SWEEP)
};

template <int SIM, int NV, int LPS, int MAPMODE, bool PACKED>
void launch_sweep_t(rn_ctx *ctx, const SweepArgs &a, hipStream_t st) {
    ProfScope prof(ctx, RN_K_SWEEP_MAP, a.n * a.n_images, st);
    const size_t lds = sweep_lds(ctx->p, MAPMODE == 3 ? 3 : 1);
    lds_opt_in(ctx, (const void *)k_sweep_map<SIM, NV, LPS, MAPMODE, PACKED>, lds);
    hipLaunchKernelGGL((k_sweep_map<SIM, NV, LPS, MAPMODE, PACKED>),
                       dim3(sweep_blocks(a.n), a.n_images), dim3(SWEEP_BLOCK), lds, st,
                       ctx->p, a.n, a.ray_idxs, a.fv, a.P, a.P_inv, a.cc, a.starts, a.ends, a.S_in,
                       ctx->axes, a.vox, a.rvc, a.S_planes, a.S_voxel, a.depth_from_planes,
                       a.points, a.order, a.fv_table, a.cam_stride, a.rows_per_image, a.seg,
                       a.msgs_out, a.prior, reinterpret_cast<float4 *>(a.zero),
                       a.zero ? (int)(acc_floats(ctx) / 4) : 0, a.xcd_chunk);
}

// k_sweep_map_packed: RPW rays per wavefront (D <= 64 / RPW)
template <int NV, int LPS, int MAPMODE, bool PACKED, int RPW>
void launch_sweep_packed_t(rn_ctx *ctx, const SweepArgs &a, hipStream_t st) {
    ProfScope prof(ctx, RN_K_SWEEP_MAP, a.n * a.n_images, st);
    const size_t lds = sweep_lds(ctx->p, MAPMODE == 3 ? 3 : 1, RPW);
    lds_opt_in(ctx, (const void *)k_sweep_map_packed<NV, LPS, MAPMODE, PACKED, RPW>, lds);
    const int nwaves = (a.n + RPW - 1) / RPW;
    hipLaunchKernelGGL((k_sweep_map_packed<NV, LPS, MAPMODE, PACKED, RPW>),
                       dim3(sweep_blocks(nwaves), a.n_images), dim3(SWEEP_BLOCK), lds, st,
                       ctx->p, a.n, a.ray_idxs, a.fv, a.P, a.P_inv, a.cc, a.starts, a.ends,
                       ctx->axes, a.vox, a.rvc, a.S_planes, a.S_voxel, a.depth_from_planes,
                       a.points, a.order, a.fv_table, a.cam_stride, a.rows_per_image, a.seg,
                       a.msgs_out, a.prior, reinterpret_cast<float4 *>(a.zero),
                       a.zero ? (int)(acc_floats(ctx) / 4) : 0,
                       a.xcd_chunk > 0 ? (a.xcd_chunk + RPW - 1) / RPW : 0);
}

// pick the plane-sweep flavour: cooperative for F=32 and 2..9 views (two / four rays per
// wavefront for D <= 32 / 16 unless rn_options.sweep_rays_per_wave says 1), generic otherwise
template <int MAPMODE, bool PACKED>
void launch_sweep(rn_ctx *ctx, const SweepArgs &a, bool have_features, hipStream_t st) {
    if (!have_features) {
        launch_sweep_t<0, 1, 8, MAPMODE, PACKED>(ctx, a, st);
        return;
    }
    const bool cooperative = ctx->p.F == 32 && !ctx->generic_sweep &&
        with_value<2, 3, 4, 5, 6, 7, 8, 9>(ctx->p.N, [&](auto nv) {
            with_value<1, 2, 4>(sweep_rays_per_wave(ctx), [&](auto rpw) {
                constexpr int NV = decltype(nv)::value, RPW = decltype(rpw)::value;
                if constexpr (RPW == 1)
                    launch_sweep_t<2, NV, 8 / SWEEP_V4, MAPMODE, PACKED>(ctx, a, st);
                else
                    launch_sweep_packed_t<NV, 8 / SWEEP_V4, MAPMODE, PACKED, RPW>(ctx, a, st);
            });
        });
    if (!cooperative) launch_sweep_t<1, 1, 8, MAPMODE, PACKED>(ctx, a, st);
}

// ---- sampling schemes (include/raynet_hip.h, "sampling schemes") ----
// the host POD checked and turned into the kernels' argument; RN_OK or a recorded failure
int scheme_args(rn_ctx *ctx, const rn_sampling *sm, const char *what, SchemeArgs &sa) {
    if (!sm) return fail(ctx, RN_ERR_INVALID, "%s: sampling is required", what);
    if (sm->scheme != RN_SAMPLE_IN_BBOX && sm->scheme != RN_SAMPLE_IN_RANGE &&
        sm->scheme != RN_SAMPLE_IN_DISPARITY)
        return fail(ctx, RN_ERR_INVALID, "%s: unknown sampling scheme %d", what, (int)sm->scheme);
    if (ctx->p.D < 2) return fail(ctx, RN_ERR_INVALID, "%s: D = %d, a scheme needs D >= 2", what, ctx->p.D);
    const float r0 = sm->range[0], r1 = sm->range[1];
    if (sm->scheme == RN_SAMPLE_IN_RANGE && !(r0 > 0.0f && r0 < r1 && r1 < INFINITY))
        return fail(ctx, RN_ERR_INVALID, "%s: depth range (%g, %g) is not 0 < r0 < r1 < infinity",
                    what, (double)r0, (double)r1);
    sa.id = sm->scheme;
    sa.r0 = r0;
    sa.r1 = r1;
    for (int i = 0; i < 12; i++) {
        sa.far_cam[i] = sm->far_P_inv[i];
        sa.far_cam[16 + i] = sm->far_P[i];
    }
    for (int i = 0; i < 4; i++) sa.far_cam[12 + i] = sm->far_centre[i];
    return RN_OK;
}

// K9 / K10 under sample_in_disparity: cooperative for F = 32 and 2..9 views, generic otherwise;
// one ray per wavefront whatever D is
void launch_sweep_disparity(rn_ctx *ctx, int n, const int32_t *ray_idxs, const float *features,
                            const float *P, const float *P_inv, const float *cc,
                            const SchemeArgs &sa, float *Sp, float *depth_map, float *points,
                            hipStream_t st) {
    ProfScope prof(ctx, RN_K_SWEEP_MAP, n, st);
    const FeatureViews fv = stacked_views(ctx->p, features);
    const size_t lds = sizeof(float) * (size_t)SWEEP_WAVES * ctx->p.D;
    auto go = [&](auto kernel) {
        lds_opt_in(ctx, (const void *)kernel, lds);
        hipLaunchKernelGGL(kernel, dim3(sweep_blocks(n)), dim3(SWEEP_BLOCK), lds, st, ctx->p, n,
                           ray_idxs, fv, P, P_inv, cc, sa, Sp, depth_map, points);
    };
    const bool cooperative = ctx->p.F == 32 && !ctx->generic_sweep &&
        with_value<2, 3, 4, 5, 6, 7, 8, 9>(ctx->p.N, [&](auto nv) {
            go(k_sweep_disparity<2, decltype(nv)::value>);
        });
    if (!cooperative) go(k_sweep_disparity<1, 1>);
}
// K9 / K10 under sample_in_range: the ray's segment (k_range_segments, into a buffer the context
// keeps), then the plane sweep the old entries run, on segments instead of on pixels -- the same
// kernels, the packed D <= 32 layout included
int launch_sweep_range(rn_ctx *ctx, int n, const int32_t *ray_idxs, const float *features,
                       const float *P, const float *P_inv, const float *cc, const SchemeArgs &sa,
                       float *Sp, float *depth_map, float *points, hipStream_t st) {
    if ((size_t)n > ctx->range_seg_rays) {
        if (ctx->range_seg) RN_HIP(ctx, hipFree(ctx->range_seg));      // (waits for its readers)
        ctx->range_seg = nullptr;
        ctx->range_seg_rays = 0;
        RN_HIP(ctx, hipMalloc(&ctx->range_seg, sizeof(float) * 6 * (size_t)n));
        ctx->range_seg_rays = (size_t)n;
    }
    float *starts = ctx->range_seg, *ends = ctx->range_seg + 3 * (size_t)n;
    {
        ProfScope prof(ctx, RN_K_OTHER, n, st);
        hipLaunchKernelGGL(k_range_segments, dim3(thread_blocks(n)), dim3(BLOCK), 0, st, ctx->p, n,
                           ray_idxs, P_inv, cc, sa.r0, sa.r1, starts, ends);
    }
    SweepArgs a{n, nullptr, stacked_views(ctx->p, features), P, nullptr, cc, starts, ends, nullptr,
                nullptr, nullptr, Sp, nullptr, depth_map, points};
    launch_sweep<0, false>(ctx, a, true, st);
    return RN_OK;
}
inline int launch_sweep_scheme(rn_ctx *ctx, int n, const int32_t *ray_idxs, const float *features,
                               const float *P, const float *P_inv, const float *cc,
                               const SchemeArgs &sa, float *Sp, float *depth_map, float *points,
                               hipStream_t st) {
    if (sa.id == SCHEME_RANGE)
        return launch_sweep_range(ctx, n, ray_idxs, features, P, P_inv, cc, sa, Sp, depth_map, points, st);
    launch_sweep_disparity(ctx, n, ray_idxs, features, P, P_inv, cc, sa, Sp, depth_map, points, st);
    return RN_OK;
}

// the slab-box rows that describe `vox` (a pointer into the bound list buffer), or null
inline int2 *slab_boxes_for(const rn_ctx *ctx, const int32_t *vox, int64_t n, bool need_valid) {
    if (!ctx->sb_boxes || !vox || vox < ctx->sb_vox) return nullptr;
    const int64_t off = vox - ctx->sb_vox;
    if (off % ctx->p.M) return nullptr;
    const int64_t row0 = off / ctx->p.M;
    if (row0 % WAVE || row0 + n > ctx->sb_rows) return nullptr;
    if (need_valid && (row0 < ctx->sb_valid_lo || row0 + n > ctx->sb_valid_hi)) return nullptr;
    return ctx->sb_boxes + (row0 / WAVE) * slab_box_count(ctx->p.M);
}

// workgroups per box-scatter tile (grid.y): enough of them for ~16 per CU
inline int box_split(int n, int tile_rays) {
    constexpr int TARGET = 4096, MOST = 4;
    const int tiles = (n + tile_rays - 1) / tile_rays;
    return max(1, min(MOST, TARGET / max(tiles, 1)));
}

// how a sweep reads its accumulator and what it clears on the side (the plan path, rn_scene_run)
struct AccMode {
    bool uniform = false;      // every voxel holds acc_in[0]
    bool biased = false;       // acc_in holds sums only: the prior `bias` is added at the gather
    float bias = 0.0f;
    float *zero = nullptr;     // cleared by the FIRST k_bp launch of this call (rn_acc_size floats)
};

template <bool PACKED, bool CLIP_IN>
void launch_bp_kernel(rn_ctx *ctx, int n, const float *Sv, const int32_t *vox, const int32_t *rvc,
                      const float *acc_in, const float *msgs_in, float *msgs_out, hipStream_t st,
                      const AccMode &am, bool clear) {
    ProfScope prof(ctx, RN_K_BP, n, st);
    float4 *zero = clear ? reinterpret_cast<float4 *>(am.zero) : nullptr;
    const int zero4 = zero ? (int)(acc_floats(ctx) / 4) : 0;
    // the plan path's iterations after the first: everything the kernel would test per chunk
    // is known here (k_bp's STEADY)
    const bool steady = PACKED && !CLIP_IN && msgs_in && !am.uniform && am.biased;
    with_chunks((ctx->p.M + WAVE - 1) / WAVE, [&](auto nch) {
        with_bool(steady, [&](auto sy) {
            hipLaunchKernelGGL((k_bp<decltype(nch)::value, PACKED, CLIP_IN, decltype(sy)::value>),
                               dim3(ray_blocks_mrf(n)), dim3(RAY_BLOCK), 0, st, ctx->p, n, Sv, vox,
                               rvc, acc_in, msgs_in, msgs_out, am.uniform ? 1 : 0, am.bias,
                               am.biased ? 1 : 0, zero, zero4);
        });
    });
}

// the scatter kernel for `level` (see BoxPolicy) over rows [0, n)
template <bool PACKED>
void launch_scatter_kernel(rn_ctx *ctx, int n, const float *msgs, const int32_t *vox,
                           const int32_t *rvc, void *acc_out, hipStream_t st, int level,
                           bool fixed) {
    ProfScope prof(ctx, RN_K_SCATTER, n, st);
    // a work list bound for exactly these rows and this tile shape (else: tiles x box_split)
    const int32_t *items = PACKED && ctx->sc_items && vox == ctx->sc_vox && n == ctx->sc_rows &&
                           level == ctx->sc_level ? ctx->sc_items : nullptr;
    // tiles of RAYS x STEPS with an LDS box of `cap` voxels
    auto box = [&](auto rays, auto steps, int cap) {
        constexpr int RAYS = decltype(rays)::value, STEPS = decltype(steps)::value;
        with_bool(fixed, [&](auto fx) {
            hipLaunchKernelGGL((k_scatter_box<PACKED, RAYS, STEPS, decltype(fx)::value>),
                               items ? dim3(ctx->sc_count, 1)
                                     : dim3((n + RAYS - 1) / RAYS, box_split(n, RAYS)),
                               dim3(BLOCK), cap * sizeof(double), st, ctx->p, n, msgs, vox, rvc,
                               acc_out, ctx->box_stats, cap,
                               (const int2 *)(PACKED ? slab_boxes_for(ctx, vox, n, true) : nullptr),
                               items);
        });
    };
    if (level == 0) {
        box(int_c<128>{}, int_c<32>{}, 4096);
    } else if (level == 1) {
        box(int_c<256>{}, int_c<16>{}, 6144);
    } else if (fixed) {
        hipLaunchKernelGGL((k_scatter_direct_fixed<PACKED>), dim3(ray_blocks(n)), dim3(BLOCK), 0, st,
                           ctx->p, n, msgs, vox, rvc, static_cast<unsigned long long *>(acc_out));
    } else {
        hipLaunchKernelGGL((k_scatter_slab<PACKED>),
                           dim3(((n + WAVE - 1) / WAVE) *
                                ((ctx->p.M + SLAB_STEPS - 1) / SLAB_STEPS)),
                           dim3(WAVE), 0, st, ctx->p, n, msgs, vox, rvc,
                           static_cast<float *>(acc_out));
    }
}

// One BP sweep: k_bp (messages) + the accumulator scatter that fits the row layout.
template <bool PACKED, bool CLIP_IN>
int launch_bp(rn_ctx *ctx, int n, const float *Sv, const int32_t *vox, const int32_t *rvc,
              const float *acc_in, const float *msgs_in, void *acc_out, float *msgs_out,
              hipStream_t st, bool patch_rows = false, bool fixed = false,
              const AccMode &am = AccMode(), bool skip_bp = false) {
    // patch-ordered rows take the LDS-box scatter, at the tile shape its overflow counters ask for
    constexpr int LAST = BoxPolicy::LAST;
    int level = ctx->scatter_mode == 0 ? LAST : (ctx->scatter_mode == 2 || patch_rows) ? 0 : LAST;
    if (level == 0) level = ctx->box.observe(ctx->box_stats_host[0], ctx->box_stats_host[1]);
    // k_bp is bound by VALU issue and its dependent row / gather round trips, the box scatter
    // by LDS atomics and barriers: with the rows in two halves the scatter of the first half
    // runs (on the context's second stream) while the second half's messages are computed.
    const size_t M = (size_t)ctx->p.M, VW = PACKED ? 1 : 3;
    const bool split = ctx->overlap == 1 || (ctx->overlap == 2 && level >= 1 && level < LAST);
    const int nA = split && PACKED && n >= 65536 && !skip_bp ? (n / 2 + 255) / 256 * 256 : n;
    if (!skip_bp) {     // (else: the plane sweep wrote the messages and cleared am.zero)
        launch_bp_kernel<PACKED, CLIP_IN>(ctx, nA, Sv, vox, rvc, acc_in, msgs_in, msgs_out, st, am, true);
        RN_LAUNCH_CHECK(ctx);
    }
    if (nA < n) {
        RN_HIP(ctx, hipEventRecord(ctx->ev_fork, st));
        launch_bp_kernel<PACKED, CLIP_IN>(ctx, n - nA, Sv + nA * M, vox + nA * M * VW, rvc + nA, acc_in,
                                          msgs_in ? msgs_in + nA * M : nullptr, msgs_out + nA * M, st,
                                          am, false);
        RN_LAUNCH_CHECK(ctx);
        RN_HIP(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
        launch_scatter_kernel<PACKED>(ctx, nA, msgs_out, vox, rvc, acc_out, ctx->aux, level, fixed);
        RN_LAUNCH_CHECK(ctx);
        RN_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->aux));
        launch_scatter_kernel<PACKED>(ctx, n - nA, msgs_out + nA * M, vox + nA * M * VW, rvc + nA,
                                      acc_out, st, level, fixed);
        RN_LAUNCH_CHECK(ctx);
        RN_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_join, 0));
    } else {
        launch_scatter_kernel<PACKED>(ctx, n, msgs_out, vox, rvc, acc_out, st, level, fixed);
        RN_LAUNCH_CHECK(ctx);
    }
    if (ctx->box.launched(level))
        (void)hipMemcpyAsync(ctx->box_stats_host, ctx->box_stats, 2 * sizeof(unsigned),
                             hipMemcpyDeviceToHost, st);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

// the statistics planes of a depth sweep (k_depth_stats), indexed as its depth map is; none: k_depth
struct DepthStats {
    float *planes = nullptr;
    int64_t stride = 0;
};
template <bool PACKED, bool CLIP_IN>
int launch_depth(rn_ctx *ctx, int n, const float *Sv, const int32_t *vox, const int32_t *rvc,
                 const float *acc, const float *msgs, const float *cc, float *S_new,
                 float *depth_map, hipStream_t st, int rays_per_center = 0,
                 const AccMode &am = AccMode(), int cc_stride = 4,
                 const DepthDest &dest = DepthDest(), const DepthStats &stats = DepthStats()) {
    ProfScope prof(ctx, RN_K_DEPTH, n, st);
    // (k_depth's STEADY form -- its flags known at compile time, as k_bp's: slower with plain
    // row loads, 0.746 -> 0.772 ms per step, faster with the non-temporal ones, 0.717 -> 0.699)
    const bool steady = PACKED && !CLIP_IN && msgs && !S_new && depth_map && am.biased;
    if constexpr (PACKED && !CLIP_IN) {
        if (stats.planes) {
            if (!depth_map || !cc)
                return fail(ctx, RN_ERR_INVALID, "depth statistics need the depth map and the camera centre");
            with_chunks((ctx->p.M + WAVE - 1) / WAVE, [&](auto nch) {
                with_bool(steady, [&](auto sy) {
                    hipLaunchKernelGGL((k_depth_stats<decltype(nch)::value, CLIP_IN, decltype(sy)::value>),
                                       dim3(ray_blocks_mrf(n)), dim3(RAY_BLOCK), 0, st, ctx->p, n, Sv,
                                       vox, rvc, acc, msgs, ctx->axes, cc, S_new, depth_map,
                                       rays_per_center, am.bias, am.biased ? 1 : 0, cc_stride, dest,
                                       stats.planes, stats.stride);
                });
            });
            RN_LAUNCH_CHECK(ctx);
            return RN_OK;
        }
    } else if (stats.planes) {
        return fail(ctx, RN_ERR_INVALID, "depth statistics: resident (packed, clipped) rows only");
    }
    with_chunks((ctx->p.M + WAVE - 1) / WAVE, [&](auto nch) {
        with_bool(steady, [&](auto sy) {
            hipLaunchKernelGGL((k_depth<decltype(nch)::value, PACKED, CLIP_IN, decltype(sy)::value>),
                               dim3(ray_blocks_mrf(n)), dim3(RAY_BLOCK), 0, st, ctx->p, n, Sv, vox,
                               rvc, acc, msgs, ctx->axes, cc, S_new, depth_map, rays_per_center,
                               am.bias, am.biased ? 1 : 0, cc_stride, dest);
        });
    });
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

inline AccMode uniform_mode(bool uniform) {
    AccMode am;
    am.uniform = uniform;
    return am;
}

int need_axes(rn_ctx *ctx) {
    if (!ctx->have_axes)
        return fail(ctx, RN_ERR_STATE, "rn_set_voxel_grid must be called before this entry point");
    return RN_OK;
}

}  // namespace
