/*
 * raynet_hip.h -- C ABI of libraynet_hip.so: RayNet's forward_pass hot path on
 * MI355X (gfx950).  This is the drop-in boundary.
 *
 * The reference has no C ABI: its operator interface is the set of PyCUDA
 * closure factories in raynet/cuda_implementations/ (one .py per kernel family), each of which wraps one
 * `prepared_call` of a __global__ kernel.  Every entry point below replaces one
 * of those launches (kernel numbers K1..K12 as in SURVEY.md section 2.2); the
 * comment above each function names the reference launcher (file:line) it
 * stands in for.  INTEGRATION.md shows the ctypes stub a maintainer would put
 * in place of each PyCUDA closure.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     the name ends in _host;
 *   - the caller allocates every buffer and keeps it alive; the library never
 *     allocates per call and never frees caller memory (reference: `to_gpu` in
 *     the driver, raynet/forward_pass.py:515-538);
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as
 *     void*; NULL = the null stream); no hidden global state, one rn_ctx per
 *     device;
 *   - return value: RN_OK or a negative rn_status; no exceptions cross the
 *     boundary.  The Python mirror re-raises shape/dtype problems as
 *     AssertionError like the reference (raynet_fp.py:291-301);
 *   - msgs_in and msgs_out may alias (the reference always aliases them,
 *     raynet_fp.py:321-323, mrf_cuda.py:73-75);
 *   - there is NO CPU fallback in this library.  rn_create fails with
 *     RN_ERR_NO_DEVICE when no gfx950 device is visible.
 *
 * Array layouts are the reference's:
 *   features   [N][H+padding+1][W+padding+1][F] f32   (forward_pass.py:622-641)
 *   P          [N][3][4] f32, P_inv [4][3] f32, camera_center [4] f32
 *   voxel_grid [gx][gy][gz][3] f32                     (forward_pass.py:573-575)
 *   ray_idxs   [n] i32, ray_idx = x*H + y              (sampling_schemes.cu:5-8)
 *   rvi        [n][M][3] i32, rvc [n] i32
 *   S (planes) [n][D] f32, S_voxel / msgs / S_new [n][M] f32
 *   acc        [gx][gy][gz] f32 (log-odds)
 */
#ifndef RAYNET_HIP_H
#define RAYNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RN_OK = 0,
    RN_ERR_INVALID = -1,     /* bad argument / unsupported size          */
    RN_ERR_HIP = -2,         /* a HIP runtime call failed                */
    RN_ERR_NO_DEVICE = -3,   /* no usable gfx950 device                  */
    RN_ERR_STATE = -4        /* call order (e.g. voxel grid not set)     */
} rn_status;

/* The values the reference bakes into its kernels as $literals
 * (cuda_implementations/raynet_fp.py:230-248); here they are run-time. */
typedef struct {
    int32_t M;        /* generation_params.max_number_of_marched_voxels */
    int32_t D;        /* depth_planes                                    */
    int32_t N;        /* neighbors + 1                                   */
    int32_t F;        /* feature channels                                */
    int32_t H;        /* image height                                    */
    int32_t W;        /* image width                                     */
    int32_t padding;  /* generation_params.padding                       */
    int32_t grid[3];  /* voxel grid shape                                */
    float bbox[6];    /* scene.bbox: min xyz, max xyz                    */
    int32_t device;   /* HIP device ordinal                              */
} rn_config;

typedef struct rn_ctx rn_ctx;

/* perform_raynet_fp(M,D,N,F,H,W,padding,bbox,grid_shape,"sample_in_bbox")
 * (raynet_fp.py:10-21): where the reference JIT-compiles, this validates the
 * configuration and creates a context. */
int rn_create(const rn_config *cfg, rn_ctx **out);
void rn_destroy(rn_ctx *ctx);

/* Behaviour options of a context -- schedule and A/B knobs; no result depends on them beyond
 * the summation order of the accumulator scatter.  The Python mirror is
 * raynet_amd.hip_implementations.options.PathOptions; the reference has no counterpart (its
 * only launch knob is `threads=2048`, raynet_fp.py:288).  rn_create starts from the defaults
 * below, overridden by the environment variables named here (read there and nowhere else). */
typedef struct {
    int32_t scatter_mode;   /* -1 by row layout (default), 0 slab scatter, 2 LDS-box scatter
                               [RAYNET_HIP_SCATTER_MODE] */
    int32_t box_level;      /* tile shape the adaptive box scatter starts from: 0 (default) 128
                               rays x 32 steps, 1: 256 x 16, 2: slab scatter [RAYNET_HIP_BOX_LEVEL] */
    int32_t box_pin;        /* != 0: stay at box_level [RAYNET_HIP_BOX_PIN] */
    int32_t overlap;        /* second stream (scatter || BP halves, traversal || plane sweep): 0 off,
                               1 on, 2 (default) when the scatter runs at level 1 [RAYNET_HIP_OVERLAP] */
    int32_t generic_sweep;  /* != 0: the reference-order plane sweep even for F = 32
                               [RAYNET_HIP_GENERIC_SWEEP] */
    int32_t sweep_rays_per_wave;  /* rays one wavefront of the cooperative plane sweep takes: 0
                               (default) by D -- 4 for D <= 16, 2 for D <= 32, else 1; 1: always one
                               (the same bits, slower for D <= 32) [RAYNET_HIP_SWEEP_RAYS_PER_WAVE] */
} rn_options;
int rn_get_options(const rn_ctx *ctx, rn_options *out);
/* also restarts the adaptive scatter (rn_scatter_reset) */
int rn_set_options(rn_ctx *ctx, const rn_options *opt);
const char *rn_last_error(const rn_ctx *ctx);
const char *rn_version(void);

/* Voxel centres are read by K1/K2/K6/K11/K12 from the [gx][gy][gz][3] array
 * (planes_voxels_mapping.cu:52-57).  The grid is separable, so the context keeps
 * the three per-axis centre tables extracted from the caller's array (bit-equal
 * values, 1.5 KB instead of 25 MB of gathers).  Call once per scene. */
int rn_set_voxel_grid(rn_ctx *ctx, const float *voxel_grid, void *stream);

/* GPUArray.fill (forward_pass.py:646-648, :678) */
int rn_fill_f32(rn_ctx *ctx, float *dst, int64_t count, float value, void *stream);
int rn_fill_i32(rn_ctx *ctx, int32_t *dst, int64_t count, int32_t value, void *stream);

/* ---- stand-alone stages ------------------------------------------------ */

/* sample_in_bbox for a list of rays -> ray_start/ray_end [n][3]
 * (sampling_schemes.cu:44-90; what every fused kernel does first). */
int rn_sample_rays(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *P_inv,
                   const float *camera_center, float *ray_start, float *ray_end,
                   void *stream);

/* K8 batch_sample_points_in_bbox, launcher sample_points.py:12-54:
 * points [n][D][4] */
int rn_sample_points(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *P_inv,
                     const float *camera_center, float *points, void *stream);

/* K7 batch_compute_similarities (feature_similarities.cu:126-146): S [n][D] */
int rn_compute_similarities(rn_ctx *ctx, int32_t n, const float *features, const float *P,
                            const float *ray_start, const float *ray_end, float *S,
                            void *stream);

/* K5 batch_voxel_traversal, launcher ray_tracing_cuda.py:35-63 */
int rn_voxel_traversal(rn_ctx *ctx, int32_t n, const float *ray_start, const float *ray_end,
                       int32_t *rvi, int32_t *rvc, void *stream);

/* K6 batch_planes_voxels_mapping, launcher planes_voxels_mapping_cuda.py:28-65 */
int rn_planes_to_voxels(rn_ctx *ctx, int32_t n, const int32_t *rvi, const int32_t *rvc,
                        const float *ray_start, const float *ray_end, const float *S,
                        float *S_new, void *stream);

/* K3 batch_belief_propagation, launcher mrf_cuda.py:37-79.
 * msgs_in may be NULL: all-zero messages (then msgs_out is only written). */
int rn_bp_sweep(rn_ctx *ctx, int32_t n, const float *S, const int32_t *rvi, const int32_t *rvc,
                const float *acc_in, const float *msgs_in, float *acc_out, float *msgs_out,
                void *stream);

/* K4 batch_depth_estimation, launcher mrf_cuda.py:81-122 */
int rn_depth_estimation(rn_ctx *ctx, int32_t n, const float *S, const int32_t *rvi,
                        const int32_t *rvc, const float *acc, const float *msgs, float *S_new,
                        void *stream);

/* ---- fused kernels of the forward-pass drivers -------------------------- */

/* K9 batch_multi_view_cnn_forward_pass, launcher similarities.py:101-130:
 * sample + plane sweep -> S [n][D] */
int rn_mvcnn_similarities(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                          const float *P, const float *P_inv, const float *camera_center,
                          float *S, void *stream);

/* K10 batch_multi_view_cnn_forward_pass_with_depth, launcher similarities.py:252-285:
 * K9 + arg-max plane -> depth_map [n]; points [n][D][4] is filled too */
int rn_mvcnn_depth(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                   const float *P, const float *P_inv, const float *camera_center, float *S,
                   float *points, float *depth_map, void *stream);

/* K11 batch_mvcnn_planes_voxels_with_ray_marching, launcher
 * mvcnn_with_ray_marching_and_voxels_mapping.py:137-174 */
int rn_mvcnn_voxel_space(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                         const float *P, const float *P_inv, const float *camera_center,
                         int32_t *rvi, int32_t *rvc, float *S_voxel, void *stream);

/* K12 ..._with_depth, launcher mvcnn_with_ray_marching_and_voxels_mapping.py:339-378 */
int rn_mvcnn_voxel_space_depth(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs,
                               const float *features, const float *P, const float *P_inv,
                               const float *camera_center, int32_t *rvi, int32_t *rvc,
                               float *S_voxel, float *depth_map, void *stream);

/* K1 batch_raynet_fp, launcher raynet_fp.py:274-326 */
int rn_fused_bp_sweep(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                      const float *P, const float *P_inv, const float *camera_center,
                      int32_t *rvi, int32_t *rvc, float *S_voxel, const float *acc_in,
                      const float *msgs_in, float *acc_out, float *msgs_out, void *stream);

/* K2 batch_complete_depth_estimation, launcher raynet_fp.py:328-376 */
int rn_fused_depth(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                   const float *P, const float *P_inv, const float *camera_center,
                   int32_t *rvi, int32_t *rvc, float *S_voxel, const float *acc,
                   const float *msgs, float *depth_map, void *stream);

/* ---- resident-scene path (what RayNetForwardPass runs on MI355X) -------- *
 * The reference recomputes features, similarities, traversal and mapping in
 * each of its 3 BP sweeps and again in the depth sweep (forward_pass.py:593-664,
 * :682-736) and round-trips messages through host memory.  With 288 GB of HBM
 * the per-ray state stays resident instead: rn_scene_prepare runs the
 * K1-prefix once per reference image and keeps, per ray, the packed voxel list
 * and the clipped+renormalised voxel-space column; the sweeps then stream it.
 * Results are those of K1/K2 called with the same inputs.
 *   vox  [n][M] i32  packed (x<<20 | y<<10 | z)
 *   Sr   [n][M] f32  clip_and_renorm(S_voxel) (mrf_bp.cu:103-111); the row of a ray with
 *                    rvc <= 1 is NOT written (such a ray sends no message and its depth is
 *                    that of its only voxel, mrf_np.py:300: nothing reads its column)
 * features_views: N device pointers (HOST array), one [Hf][Wf][F] map per view,
 * so a bank of per-view feature maps needs no re-stacking per reference image.
 * order (optional, may be NULL): a permutation of 0..n-1; wavefront i of the plane
 * sweep works on ray order[i].  It changes nothing but the schedule: walking the
 * rays along the direction of the epipolar lines keeps the neighbour views'
 * feature rows in L2.
 * ray_segments (optional scratch, may be NULL): [n][8] f32; the traversal leaves every
 * ray's bbox entry / exit point there and the plane sweep reads it back instead of
 * repeating the double-precision back-projection (sampling_schemes.cu:44-90) per wavefront. */
int rn_scene_prepare(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs,
                     const float *const *features_views_host, const float *P,
                     const float *P_inv, const float *camera_center, const int32_t *order,
                     int32_t *vox, int32_t *rvc, float *Sr, float *ray_segments, void *stream);

/* The same for ALL reference images of a scene in two launches (one grid row per image).
 * Image g owns rows [g*rows_per_image, g*rows_per_image + n) of vox / rvc / Sr; all images
 * share ray_idxs [n] and the optional schedule `order` [n].
 *   cameras        [n_images][12N + 12 + 4] f32: P of the N views, P_inv and camera centre
 *                  of the reference view (device)
 *   features_views [n_images][N] device pointers, stored in DEVICE memory
 *   ray_segments   optional scratch [n_images * rows_per_image][8] f32 (see above) */
int rn_scene_prepare_all(rn_ctx *ctx, int32_t n_images, int32_t n, int64_t rows_per_image,
                         const int32_t *ray_idxs, const float *const *features_views,
                         const float *cameras, const int32_t *order, int32_t *vox, int32_t *rvc,
                         float *Sr, float *ray_segments, void *stream);

/* Slab boxes (optional).  The accumulator scatter of RN_ROWS_PATCHES rows sums a tile's
 * messages in an LDS image of the bounding box of the voxels the tile's rays visit in a chunk
 * of steps.  That box depends on the rays alone, not on the messages: bound to a list buffer,
 * rn_scene_prepare_all leaves, per 64 consecutive rows and per 16 steps, the box of the voxels
 * those rays visit there (a DDA is monotone along every axis: the extremes are the first and
 * the last voxel), and the three scatters of a pass merge boxes instead of scanning the lists.
 *   vox    the buffer rn_scene_prepare_all writes its lists to ([rows][M] i32)
 *   boxes  rn_slab_boxes_size(rows) i32 of scratch owned by the caller
 * Contract: while bound, the rows of `vox` are written by rn_scene_prepare_all only
 * (rn_scene_prepare into the buffer switches the table off until the next prepare_all);
 * rn_scene_bp_sweep* use the table for list pointers inside `vox` whose rows it covers, and
 * scan the lists as before for any other pointer.  boxes == NULL unbinds. */
int64_t rn_slab_boxes_size(const rn_ctx *ctx, int64_t rows);
int rn_scene_bind_slab_boxes(rn_ctx *ctx, const int32_t *vox, int64_t rows, int32_t *boxes);

/* Work list of the LDS-box scatter for the rows [0, rows) of the list buffer `vox` at tile level
 * `level` (0: 128 rays x 32 steps, 1: 256 x 16): items[i] = tile << 12 | first chunk << 6 | chunks
 * -- one workgroup per item, in the list's order (the caller sorts longest first and never lists
 * a chunk no ray of its tile reaches; every (tile, chunk) below the tile's longest ray must be in
 * exactly one item).  A scatter launch over exactly these rows at that level takes the list;
 * any other launch -- and every launch after items == NULL -- deals tiles x chunks out itself.
 * The list depends on the rays' voxel counts only (ray_tracing.pyx:64-199), not on messages: it
 * is built once per scene and shard.  Speed only: the sums are the same.  The tile field has 19
 * bits: rows beyond 2^19 tiles of the level are refused (RN_ERR_INVALID). */
int rn_scene_bind_scatter_items(rn_ctx *ctx, const int32_t *vox, int64_t rows, int32_t level,
                                const int32_t *items, int32_t count);

/* What the adaptive accumulator scatter of the resident path last saw (diagnostics): the tile
 * shape in use (0: 128 rays x 32 steps, 1: 256 x 16, 2: slab scatter) and, of the launches
 * between the launcher's last two looks at the counters that have arrived on the host (they are
 * copied out for the first dozen scatters after a reset only), the number of tile chunks and how
 * many of them did not fit the LDS box. */
int rn_scatter_state(const rn_ctx *ctx, int32_t *level, uint32_t *chunks, uint32_t *overflowed);

/* 1 once the scatter no longer copies its overflow counters out (a dozen launches after
 * rn_create / rn_scatter_reset / rn_set_options): from then on no launch of the resident path
 * touches the host and the tile shape stays as it is -- the precondition for recording a step's
 * launches into a HIP graph (the reference has no counterpart: PyCUDA launches one kernel at a
 * time from the interpreter, cuda_implementations/raynet_fp.py:303-326). */
int rn_scatter_settled(const rn_ctx *ctx);

/* Voxel counts only (the traversal of rn_scene_prepare_all without its lists): rvc
 * [n_images][n] i32, row g*n + i = number of voxels ray ray_idxs[i] crosses in reference image
 * g (<= M).  The multi-GPU driver balances its ray shards by these counts (the cost of the BP
 * sweep, the scatter and the depth sweep is per traversed voxel, ray_tracing.pyx:64-199 decides
 * how many there are); cameras as in rn_scene_prepare_all. */
int rn_scene_count_voxels(rn_ctx *ctx, int32_t n_images, int32_t n, const int32_t *ray_idxs,
                          const float *cameras, int32_t *rvc, void *stream);

/* Accumulators of the resident path are stored as 4x4x4 bricks,
 * [ceil(gx/4)][ceil(gy/4)][ceil(gz/4)][4][4][4] f32 = rn_acc_size() floats (a ray stays
 * inside a brick for ~4 steps, so a wavefront's gather touches ~4x fewer cache lines than in
 * the [gx][gy][gz] array).  rn_acc_to_grid / rn_acc_from_grid convert to / from the
 * reference's [gx][gy][gz] layout (mrf_bp.cu:3-10); padding voxels are never read back.
 * acc_part: [rn_acc_copies()][rn_acc_size()] f32 partial accumulator(s) the sweep scatters
 * into, zero before the first sweep of an iteration (rn_acc_copies() is 1: per-XCD copies
 * were measured and bought nothing). */
int64_t rn_acc_size(const rn_ctx *ctx);
int rn_acc_to_grid(rn_ctx *ctx, const float *acc, float *grid_out, void *stream);
int rn_acc_from_grid(rn_ctx *ctx, const float *grid, float *acc_out, void *stream);
int rn_acc_copies(const rn_ctx *ctx);
/* first_sweep is a set of rn_sweep_flags:
 * RN_SWEEP_ZERO_MSGS   the messages are taken as zero and `msgs` is only written, so it needs
 *                      no zero-fill (the reference zero-fills for iteration 0,
 *                      forward_pass.py:613-615);
 * RN_SWEEP_UNIFORM_ACC every voxel of acc_in holds acc_in[0] (iteration 0 starts from the
 *                      prior everywhere, forward_pass.py:533-538): only that element is read,
 *                      nothing is gathered.
 * row_layout says how consecutive rows relate in the image, which only selects the
 * accumulator-scatter kernel (any value is correct for any input, it is a speed hint):
 * RN_ROWS_LINEAR  -- consecutive rows run along an image column / row (ray-index order);
 * RN_ROWS_PATCHES -- every 256 consecutive rows are a compact pixel patch (e.g. 16x16). */
typedef enum { RN_ROWS_LINEAR = 0, RN_ROWS_PATCHES = 1 } rn_row_layout;
typedef enum { RN_SWEEP_ZERO_MSGS = 1, RN_SWEEP_UNIFORM_ACC = 2 } rn_sweep_flags;
/* The scatter for RN_ROWS_PATCHES adapts its tile shape to the scene from what previous
 * sweeps measured (LDS overflow counts); call this when the scene / cameras change so that
 * the next sweeps start from the default again. */
int rn_scatter_reset(rn_ctx *ctx);
int rn_scene_bp_sweep(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                      const int32_t *rvc, const float *acc_in, float *msgs, float *acc_part,
                      int32_t first_sweep, int32_t row_layout, void *stream);
/* Deterministic mode: the same sweep, but every message is turned into a
 * signed 31.32 fixed-point integer and summed with 64-bit integer additions in LDS and in
 * acc_part_fixed [rn_acc_size()] i64 (zero before the first sweep of an iteration).  Integer
 * addition is associative: the accumulator is bit-identical from run to run, and -- with the
 * partials of several GPUs summed as int64 -- for any number of ranks.
 * rn_acc_combine_fixed: acc_out = prior + acc_part_fixed * 2^-32, and zeroes the partial. */
int rn_scene_bp_sweep_fixed(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                            const int32_t *rvc, const float *acc_in, float *msgs,
                            int64_t *acc_part_fixed, int32_t first_sweep, int32_t row_layout,
                            void *stream);
int rn_acc_combine_fixed(rn_ctx *ctx, int64_t *acc_part_fixed, float prior, float *acc_out,
                         void *stream);
/* The same on `count` elements of any slab of the accumulator: what a rank runs on ITS 1 / N of
 * the voxels between a reduce-scatter of the fixed-point partials and the all-gather of the
 * float accumulator (sharded combine; 3/4 of the all-reduce's bytes on the wire). */
int rn_acc_combine_fixed_range(rn_ctx *ctx, int64_t *acc_part_fixed, int64_t count, float prior,
                               float *acc_out, void *stream);
/* acc_out = prior + sum over copies (+ optionally `extra`, e.g. nothing or a
 * peer's partial); the copies are zeroed for the next iteration. */
int rn_acc_combine(rn_ctx *ctx, float *acc_part, float prior, float *acc_out, void *stream);
/* Only the local sum (no prior), written to acc_out; used before an all-reduce. */
int rn_acc_reduce_local(rn_ctx *ctx, float *acc_part, float *acc_out, void *stream);
int rn_acc_add_prior(rn_ctx *ctx, float *acc, float prior, void *stream);

/* depth_map [n] and, when S_new != NULL, the per-ray distribution [n][M].
 * rays_per_center > 0: the n rays are consecutive groups of rays_per_center rays (one
 * group per reference image) and group g measures its distances from
 * camera_center[4*g .. 4*g+3]; 0: one centre for all rays. */
int rn_scene_depth(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                   const int32_t *rvc, const float *acc, const float *msgs,
                   const float *camera_center, int32_t rays_per_center, float *S_new,
                   float *depth_map, void *stream);

/* The same sweep -- depth_map, S_new bit for bit as rn_scene_depth writes them -- that also
 * keeps three numbers of every ray's depth distribution before it is thrown away.  For a ray
 * with count > 1 voxels let d_i be the distribution (the row S_new gets) and
 * t_i = |centre(voxel_i) - camera_centre| in fp32, the arithmetic of the depth itself:
 *   plane 0  confidence      d_{i*}, i* the reported (first) arg-max: max_i d_i
 *   plane 1  expected depth  mu = sum_i d_i t_i
 *   plane 2  depth std       sqrt(max(0, sum_i d_i (t_i - mu)^2))
 * Rays with count <= 1 send no message and their row is all zero: confidence 0, expected depth
 * = the value depth_map gets, std 0.  stats[plane * stats_stride + ray], stats_stride >= n.
 * depth_map, camera_center and stats are required (stats == NULL is RN_ERR_INVALID, there is
 * no fallback to rn_scene_depth). */
int rn_scene_depth_stats(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *vox,
                         const int32_t *rvc, const float *acc, const float *msgs,
                         const float *camera_center, int32_t rays_per_center, float *S_new,
                         float *depth_map, float *stats, int64_t stats_stride, void *stream);

/* ---- one pass as a PLAN (what RayNetForwardPass.forward_pass enqueues per step) ----------
 * forward_pass.py:579-748 in the resident form: the caller describes the scene's buffers once
 * and then runs whole phases of a pass with one call each -- the K1 prefix of all images, one BP
 * iteration over all images, the depth sweep -- instead of one call per kernel.  Between the
 * SWEEP phases of two iterations the caller runs its exchange (the all-reduce across GPUs of
 * acc[iteration & 1], or of acc_fixed), nothing else.
 *
 * Accumulators.  Float mode: acc[0], acc[1] (rn_acc_size() floats each, bricked) hold the
 * SUM of the messages only; the prior is added where an accumulator is read (`prior + sum`,
 * the value rn_acc_combine would have stored -- bit for bit), so there is no combine kernel,
 * and the sweep of iteration t clears acc[t & 1] itself before its scatter adds into it: no
 * buffer has to be zeroed or refilled by the caller, ever (forward_pass.py:676-678's swap +
 * fill(prior) costs nothing here).  Iteration 0 reads no accumulator (the prior everywhere).
 * Deterministic mode: the scatter adds 31.32 fixed-point integers into acc_fixed (cleared by
 * RN_RUN_PREPARE and by every RN_RUN_COMBINE), RN_RUN_COMBINE turns it into acc[t & 1] =
 * prior + sum (a full log-odds accumulator), which iteration t + 1 reads as it is.
 * The depth sweep reads acc[(iterations - 1) & 1]; with iterations == 0 that is acc[1], which
 * the caller then sets itself (zeros in float mode, the prior in deterministic mode). */
typedef struct {
    int32_t n_images;              /* reference images of the pass                       */
    int32_t n;                     /* rays per image (this rank's rows of every image)   */
    int64_t rows_per_image;        /* image g owns rows [g*rows_per_image, +n); % 256 == 0 */
    const int32_t *ray_idxs;       /* [n], shared by the images                          */
    const int32_t *order;          /* optional schedule of the plane sweep, see rn_scene_prepare */
    const float *const *features_views;  /* DEVICE [n_images][N] feature-map pointers    */
    const float *cameras;          /* [n_images][12N + 16], see rn_scene_prepare_all     */
    int32_t *vox;                  /* [n_images*rows_per_image][M]                       */
    int32_t *rvc;                  /* [n_images*rows_per_image]                          */
    float *Sr;                     /* [n_images*rows_per_image][M]                       */
    float *msgs;                   /* [n_images*rows_per_image][M]                       */
    float *ray_segments;           /* optional scratch [n_images*rows_per_image][8]      */
    float *acc[2];                 /* see above                                          */
    int64_t *acc_fixed;            /* deterministic mode only, else NULL                 */
    float *depth;                  /* [n_images*rows_per_image]                          */
    float prior;                   /* log(gamma / (1 - gamma)), forward_pass.py:533-538  */
    int32_t row_layout;            /* rn_row_layout                                      */
    float *depth_image;            /* optional [n_images][depth_image_stride]: the depth sweeps
                                      write image g's map in RAY-INDEX (pixel) order,
                                      depth_image[g*stride + ray_idxs[row]], instead of depth[]
                                      in row order -- what forward_pass.py:744 hands out, with
                                      no reordering pass behind the sweep.  Entries no ray of the
                                      list maps to are left as they are                      */
    int64_t depth_image_stride;    /* floats between two images' maps (>= max ray index + 1) */
    int32_t sweep_xcd_chunk;       /* plane sweep: consecutive wavefronts (entries of `order`) in
                                      groups of this many RAYS per XCD, the groups dealt round the
                                      8 XCDs -- one group is what an XCD's private L2 sees side by
                                      side (a multiple of 4; 0: the library's default, 2048)    */
    /* depth statistics (rn_scene_depth_stats), all optional: with NULL the depth sweeps are the
       launches they are without these fields.  They go where the depths go -- */
    float *stats;                  /* ... in row order, the counterpart of `depth`:
                                      [3][n_images*rows_per_image], plane p of row r at
                                      stats[p*n_images*rows_per_image + r] (used when depth_image
                                      is NULL)                                                   */
    float *stats_image;            /* ... in pixel order, the counterpart of `depth_image` (which it
                                      needs): plane p of image g at stats_image[p*stats_image_stride
                                      + g*depth_image_stride + ray_idxs[row]]; entries no ray maps
                                      to are left as they are                                    */
    int64_t stats_image_stride;    /* floats between two planes (>= n_images*depth_image_stride) */
} rn_scene_plan;
typedef enum {
    RN_RUN_PREPARE = 1,   /* traversal + plane sweep + mapping of all images (rn_scene_prepare_all) */
    RN_RUN_SWEEP = 2,     /* BP iteration `iteration` over all images: messages + scatter          */
    RN_RUN_COMBINE = 4,   /* deterministic mode: acc[iteration & 1] = prior + acc_fixed            */
    RN_RUN_DEPTH = 8,     /* depth sweep of image `image` (all images in one launch if < 0) after
                             `iteration` BP iterations                                             */
    RN_RUN_DEPTH_RANGE = 16 /* depth sweep of `count` consecutive images from `first` in ONE launch,
                             `image` = first | count << 16: a single GPU decodes all images but
                             the last together (no launch tails between them) and the last one on
                             its own, under which the others' maps leave                         */
} rn_run_phase;
/* Runs the phases named in `phases` in the order PREPARE, SWEEP, COMBINE, DEPTH_RANGE / DEPTH.
 * (The first PREPARE | SWEEP of iteration 0 with a given prior synchronises `stream` once: the one
 * occupancy of that iteration is evaluated on the device and kept with the context.) */
int rn_scene_run(rn_ctx *ctx, const rn_scene_plan *plan, int32_t phases, int32_t iteration,
                 int32_t image, void *stream);

/* out[i] = rows[index[i]] for i < n: the depth rows of a pass (one rank's, or the ranks' blocks
 * side by side after the all-gather) into the ray-index order forward_pass.py:744 hands out.
 * `out` (16-byte aligned, like `index`) may be PAGE-LOCKED HOST memory (hipHostMalloc, torch's
 * pin_memory): the kernel then writes the map across PCIe itself -- the reordering pass and the
 * device-to-host copy (`.get()`, forward_pass.py:739-744) are one launch on `stream`. */
int rn_stitch_rows(rn_ctx *ctx, int64_t n, const float *rows, const int32_t *index, float *out,
                   void *stream);

/* ---- measurement -------------------------------------------------------- */
/* Per-launch hipEvent timing on the stream each kernel runs on.  Between
 * rn_prof_begin and rn_prof_end every kernel launch made through this context
 * is bracketed by two events; rn_prof_end synchronises and returns, per launch,
 * the kernel family (rn_kernel_id), its ray count and its duration. */
typedef enum {
    RN_K_TRAVERSE = 1,   /* voxel traversal (thread per ray)                 */
    RN_K_SWEEP_MAP = 2,  /* plane sweep + softmax (+ planes->voxels mapping) */
    RN_K_BP = 3,         /* BP sweep                                         */
    RN_K_DEPTH = 4,      /* depth estimation / arg-max                       */
    RN_K_ACC = 5,        /* accumulator combine / fill                       */
    RN_K_OTHER = 6,
    RN_K_SCATTER = 7     /* accumulator scatter of the BP messages (tile-transposed) */
} rn_kernel_id;
int rn_prof_begin(rn_ctx *ctx, int32_t capacity);
/* Which families the next rn_prof_begin brackets: bit (1 << rn_kernel_id) each, default all.
 * An event pair costs the stream a few microseconds; a timed region that wants one kernel's
 * durations only (bench.py: the dominant one) selects that family. */
int rn_prof_select(rn_ctx *ctx, uint32_t kernel_mask);
int rn_prof_end(rn_ctx *ctx, int32_t *count, int32_t *kernel_ids_host, int32_t *n_rays_host,
                float *ms_host);
/* after rn_prof_end: start of every recorded launch, in ms after the first one's start
 * (the gaps between launches = what the host side costs; tools/timeline.py) */
int rn_prof_offsets(rn_ctx *ctx, float *start_ms_host);

/* Self-test of the exact arithmetic shortcut of the index maps (raynet_kernels.h:
 * round_half_away), for tests/: out is [2][n] -- roundf(a), round_half_away(a). */
int rn_selftest_arith(rn_ctx *ctx, int32_t n, const float *a, float *out, void *stream);
/* The same for round_quotient_fast, which stands in for the two divisions of a projection
 * (feature_similarities.cu:24-25) wherever it is sure of the rounded result: out is [3][n] --
 * round_half_away(x / d), the shortcut's value, 1.0 where it is sure (elsewhere the kernels
 * take the division). */
int rn_selftest_quotient(rn_ctx *ctx, int32_t n, const float *x, const float *d, float *out,
                         void *stream);

/* The plane sweep's index arithmetic alone (feature_similarities.cu:10-61, 84-98): for every
 * ray, view and depth plane the feature vector the sweep would gather, as fy * (W + padding + 1)
 * + fx -- out [n][N][D][2]: by the generic sweep's expressions (the reference's, operation for
 * operation) and by the cooperative sweep's (rounded quotients through the reciprocal where
 * provably the same).  tests/ compares both with the reference's own NumPy `project`. */
int rn_selftest_feature_offsets(rn_ctx *ctx, int32_t n, const float *P, const float *ray_start,
                                const float *ray_end, int32_t *out, void *stream);

/* The same for the two shortcuts of the planes -> voxels mapping of the resident path
 * (raynet_kernels.h: markstein_div, plane_index_from_table), which stand in for the division
 * by |ray|^2 and for the plane walk of planes_voxels_mapping.cu:48-67.  out is [5][n]:
 * a / b (IEEE), Markstein's quotient from RN(1 / b), 1.0 where the kernels use it (b within
 * 2^-60 .. 2^60 and |a| < 2^60; the IEEE division elsewhere), the walk's plane index for clamp(t, 1e-4,
 * 1 - 1e-4) with the context's D, the table look-up's. */
int rn_selftest_mapping(rn_ctx *ctx, int32_t n, const float *a, const float *b, const float *t,
                        float *out, void *stream);

/* ---- differentiable MRF block (training) --------------
 * The reference builds this block from TensorFlow ops and lets autodiff
 * differentiate it (raynet/tf_implementations/forward_backward_pass.py:194-246,
 * raynet/mrf/mrf_tf.py:1-236); these entry points are the forward on a column that the
 * framework has already clipped + renormalised (so that step stays differentiable there)
 * and the analytic reverse-mode derivative of one BP sweep / of the depth distribution.
 * rvi is the [n][M][3] traversal output (K5 layout). */

/* left plane index and interpolation weights (c1, c2), [n][M] each, of the
 * planes->voxels mapping (planes_voxels_mapping.cu:48-84): S_voxel[i] is
 * normalise_i(c1[i] S[left[i]] + c2[i] S[left[i]+1]) */
int rn_plane_weights(rn_ctx *ctx, int32_t n, const int32_t *rvi, const int32_t *rvc,
                     const float *ray_start, const float *ray_end, int32_t *left, float *c1,
                     float *c2, void *stream);

/* rn_bp_sweep / rn_depth_estimation without their internal clip_and_renorm */
int rn_train_bp_sweep(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *rvi,
                      const int32_t *rvc, const float *acc_in, const float *msgs_in,
                      float *acc_out, float *msgs_out, void *stream);
int rn_train_depth(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *rvi,
                   const int32_t *rvc, const float *acc, const float *msgs, float *S_new,
                   void *stream);

/* Backward of rn_train_bp_sweep.  g_msgs_out [n][M]: gradient w.r.t. the new messages
 * from their direct use by the next sweep; g_acc_out [G] (may be NULL): gradient w.r.t.
 * acc_out.  Results: g_Sr [n][M] += , g_acc_in [G] += (atomic; caller zeroes),
 * g_msgs_in [n][M] = . */
int rn_train_bp_sweep_bwd(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *rvi,
                          const int32_t *rvc, const float *acc_in, const float *msgs_in,
                          const float *g_msgs_out, const float *g_acc_out, float *g_Sr,
                          float *g_acc_in, float *g_msgs_in, void *stream);

/* Backward of rn_train_depth for g_S_new [n][M]; same output conventions. */
int rn_train_depth_bwd(rn_ctx *ctx, int32_t n, const float *Sr, const int32_t *rvi,
                       const int32_t *rvc, const float *acc, const float *msgs,
                       const float *g_S_new, float *g_Sr, float *g_acc, float *g_msgs,
                       void *stream);

/* ---- consumers of the depth maps ----------------------
 * Pixel i = u*H + v (column-major, common/image.py:252-255), depth maps are [H][W] f32 as
 * the forward pass writes them (scripts/forward_pass.py:136-142); matrices and points are
 * float64 like the NumPy code these entry points restate. */

/* raynet/pointcloud.py:121-147 (_generate_points_per_image without the pixel selection):
 * points [3][H*W] f64 = centre + depth * normalised ray direction, for every pixel.
 * P_pinv [4][3], camera_center [4] (device). */
int rn_depthmap_points(rn_ctx *ctx, int32_t H, int32_t W, const double *P_pinv,
                       const double *camera_center, const float *depth_map, double *points,
                       void *stream);

/* One neighbour view of raynet/pointcloud.py:205-245: tau[i] = max(tau[i], |depth_map at the
 * point's projection - distance of the point to that camera|), inf where the projection
 * falls outside the view; first != 0 starts tau.  points [3][n] f64, P [3][4].  "Outside" is
 * decided on the rounded projection as doubles (half to even, 0 <= x < W, 0 <= y < H): a
 * projection that is NaN, +-inf or beyond any int is outside, never converted to an index.
 * A NaN depth makes tau NaN (np.maximum) until a view the point is outside of makes it inf. */
int rn_consistency_tau(rn_ctx *ctx, int32_t n, int32_t H, int32_t W, int32_t first,
                       const double *points, const double *P, const double *camera_center,
                       const float *depth_map, double *tau, void *stream);

/* Exact nearest neighbours (the KDTree.query of raynet/pointcloud.py:63-72, behind
 * Accuracy / Completeness, metrics.py:155-236): for every query point the distance to and
 * the index of the closest reference point (either output may be NULL).  Points are
 * [n][4] f32 (x, y, z, unused). */
int rn_nearest_neighbors(rn_ctx *ctx, int32_t n_ref, const float *ref_xyzw, int32_t n_query,
                         const float *query_xyzw, float *dist, int32_t *idx, void *stream);

/* ---- ground truth from scene meshes ----------------------------------------
 * The reference casts one ray per pixel through an octree of the ground-truth mesh
 * (common/scene.py:187-201, utils/oct_tree.py, utils/training_utils.py:194-220,
 * utils/fast_utils.pyx:47-117).  Here a BVH is built on the GPU (LBVH: Morton keys sorted by
 * the caller, Karras hierarchy, node boxes from the leaves' ranges) and traversed one lane
 * per ray.  Triangles are [n][9] f32 rows p0 | p1 | p2; all buffers are device memory owned
 * by the caller; nodes are [max(n-1, 1)][16] f32, leaves [n][12] f32. */

/* Build step 1 (replaces OctTree.__init__, oct_tree.py:20-38): keys[i] = 30-bit Morton code
 * of triangle i's centroid quantised in box (device, lo xyz | hi xyz) << 32 | i.  The caller
 * sorts the keys (they are unique, so the order is fixed) and hands them to rn_mesh_build. */
int rn_mesh_keys(rn_ctx *ctx, int32_t n, const float *triangles, const float *box,
                 int64_t *keys, void *stream);

/* Build step 2: leaves (p0, p1 - p0, p2 - p0, triangle index) in key order, the Karras
 * hierarchy and both child boxes of every internal node.  work: 56*n + 64 bytes of device
 * scratch.  Synchronises on `stream`; *depth_out (host) = depth of the deepest leaf;
 * RN_ERR_INVALID if it exceeds the traversal stack (63). */
int rn_mesh_build(rn_ctx *ctx, int32_t n, const float *triangles, const int64_t *sorted_keys,
                  float *nodes, float *leaves, void *work, int32_t *depth_out, void *stream);

/* get_ray_meshes_first_intersection (training_utils.py:194-220) for n rays: origins and
 * destinations [n][3] f32 -> points [n][3] f32 (the first hit, t >= 0) and tri [n] (the
 * original triangle index, -1 on a miss). */
int rn_mesh_raycast(rn_ctx *ctx, int32_t n, const float *origins, const float *destinations,
                    const float *nodes, const float *leaves, float *points, int32_t *tri,
                    void *stream);

/* RestrepoScene.get_depth_for_pixel (scene.py:187-201) for every pixel of an H x W image:
 * the ray from camera_center [3] f32 to project(P_pinv, (u, v, 1)) (P_pinv [4][3] f32, the
 * product formed in float64 and rounded once to f32); depth_map [H][W] f32 = distance of the
 * hit to the centre, 0 where the ray hits nothing. */
int rn_mesh_depthmap(rn_ctx *ctx, int32_t H, int32_t W, const float *P_pinv,
                     const float *camera_center, const float *nodes, const float *leaves,
                     float *depth_map, void *stream);

/* The nearest point of the mesh for n query points (replaces the KD-tree query of
 * raynet/pointcloud.py:63-72 behind metrics.py:155-236, which measures to the mesh's VERTICES):
 * queries [n][3] f64.  The surface is the leaves' triangles p0, p0 + e1, p0 + e2 widened to
 * float64; dist [n] f64 = the Euclidean distance to it, closest [n][3] f64 a point of the
 * returned triangle that attains it, tri [n] that triangle's original index (closest and tri
 * may be NULL).  A zero-area triangle is the segment or point it degenerates to. */
int rn_mesh_closest(rn_ctx *ctx, int32_t n, const double *queries, const float *nodes,
                    const float *leaves, double *dist, double *closest, int32_t *tri,
                    void *stream);

/* area [n] f64 = 0.5 |(p1 - p0) x (p2 - p0)| of triangles [n][9] f32, formed in float64. */
int rn_mesh_areas(rn_ctx *ctx, int32_t n, const float *triangles, double *area, void *stream);

/* n_samples stratified, area-weighted points of the surface (no counterpart in the
 * reference): area_cdf [n_triangles] f64 is the inclusive running sum of rn_mesh_areas, its
 * last entry > 0.  Sample k lies in the first triangle t with area_cdf[t] > (k + r0) /
 * n_samples * area at p0 + r1 e1 + r2 e2 ((r1, r2) folded into the triangle), formed in
 * float64 and rounded once: points [n_samples][3] f32, tri [n_samples].  r0, r1, r2 are a
 * counter-based hash of (seed, k, j). */
int rn_mesh_sample(rn_ctx *ctx, int32_t n_samples, int32_t n_triangles, const float *triangles,
                   const double *area_cdf, int64_t seed, float *points, int32_t *tri,
                   void *stream);

/* ---- point-cloud filters ------------------------------
 * The two filters the reference's evaluation puts between a cloud and its score.  Points are
 * [3][n] f64, planar, as rn_depthmap_points writes them; n == 0 is an empty launch. */

/* VoxelMask.filter (raynet/metrics.py:55-75 with keep_points_in_aabbox / point_in_aabbox,
 * utils/geometry.py:238-240, 315-348): keep [n] u8 = 1 where min <= p <= max on every axis
 * and mask[ix][iy][iz] == 1, i = rint((p - min - step / 2) / step) (half to even, like
 * np.round).  box [12] f64 (device): min xyz | max xyz | step xyz | step / 2 xyz, as NumPy
 * forms them from the float32 bounding box; mask [A][B][C] u8, C-ordered.  One deviation: on
 * the max face of an axis with an even voxel count the reference's index equals the count and
 * it raises IndexError; here the index is clamped to count - 1. */
int rn_voxel_mask(rn_ctx *ctx, int32_t n, const double *points, const double *box, int32_t A,
                  int32_t B, int32_t C, const uint8_t *mask, uint8_t *keep, void *stream);

/* ReduceDensity.filter (raynet/metrics.py:94-127), step 1 (replaces KDTree(X.T), :106, and the
 * shuffle, :102-103): keys [n] = (cx + 1) << 42 | (cy + 1) << 21 | (cz + 1) with
 * c = floor((p - lo) / h) per axis in float64 -- the caller guarantees 0 <= c <= 2^21 - 3 --
 * and the visiting priority [n], smaller = visited earlier, compared as unsigned 64-bit and
 * then by the point's index: position[i] where position (device, [n] i64: the place of point
 * i in an explicit visiting order) is given, else the counter hash
 *     mix64(mix64(seed + G) + G * (i + 1)),   G = 0x9E3779B97F4A7C15,   all modulo 2^64,
 *     mix64(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *               z ^ z >> 31   (splitmix64's output function, as rn_mesh_sample uses it). */
int rn_thin_keys(rn_ctx *ctx, int32_t n, const double *points, double lo_x, double lo_y,
                 double lo_z, double h, int64_t seed, const int64_t *position, int64_t *keys,
                 int64_t *priority, void *stream);

/* Step 2 (replaces query_radius and the loop, metrics.py:109-119): one round over the n_work
 * points work [n_work] i32 names (NULL: all n) of arrays in ascending key order -- sorted_keys
 * [n], points [3][n], priority [n], index [n] i32 (the points' original indices).  An
 * undecided point (state 0) becomes removed (2) if an earlier neighbour -- dx*dx + dy*dy +
 * dz*dz <= r2, uncontracted -- is kept (1), kept if every earlier neighbour is removed;
 * neighbours are searched in the 27 cells around it, so h > sqrt(r2).  state [n] i32 is
 * updated in place (zero it before the first round); *undecided (device i32, zeroed by the
 * caller) += the points of the work list still undecided.  Rounds repeated until that is 0
 * leave exactly the reference's kept set for the same visiting order. */
int rn_thin_round(rn_ctx *ctx, int32_t n_work, const int32_t *work, int32_t n,
                  const int64_t *sorted_keys, const double *points, const int64_t *priority,
                  const int32_t *index, double r2, int32_t *state, int32_t *undecided,
                  void *stream);

/* ---- ground-truth depth from a point cloud ----------------
 * A DTU scan ships its ground truth as one point cloud; its depth maps are the cloud's
 * z-buffer in every view (no counterpart in the reference, which reads the maps from disk). */

/* points [n_points][3] f32, cameras [n_views][21] f64 (K [3][3] | R [3][3] | t [3], row-major),
 * all device memory.  Per point and view, in float64 with every operation rounded on its own:
 *     Xc_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k,   h_k = (K_k0 Xc_0 + K_k1 Xc_1) + K_k2 Xc_2,
 *     (iu, iv) = (rint(h_0 / h_2), rint(h_1 / h_2))   (half to even),   z32 = (float) Xc_2;
 * the point counts iff 0 < h_2 < inf, Xc_2 > 0, z32 < inf, 0 <= iu < W and 0 <= iv < H (a NaN
 * fails every test).  zbuf [n_views][H][W] u32: zbuf[view][iv][iu] = min(itself, bit pattern of
 * z32) -- an unsigned minimum, which for positive floats is the float minimum.  THE CALLER
 * fills zbuf with 0x7F800000 (+inf) before the first call; the entry never clears it, so
 * several calls accumulate several chunks of a cloud into one buffer.  All views are one
 * launch: a point is read once.  n_points <= 2^30; n_points == 0 or n_views == 0 is an empty
 * launch. */
int rn_cloud_zbuffer(rn_ctx *ctx, int32_t n_points, const float *points, int32_t n_views,
                     const double *cameras, int32_t H, int32_t W, uint32_t *zbuf, void *stream);

/* The same buffer, and counts [2] u64 (device, zeroed by the caller) += the (point, view) pairs
 * that landed on a pixel | those of them whose atomic the pre-test skipped (the stored value was
 * already <= z32): the measurement of tools/cloud_depth_bench.py. */
int rn_cloud_zbuffer_counted(rn_ctx *ctx, int32_t n_points, const float *points, int32_t n_views,
                             const double *cameras, int32_t H, int32_t W, uint32_t *zbuf,
                             uint64_t *counts, void *stream);

/* ---- training batches: rays of many reference views in one launch ---- */

/* n candidate rays of ONE scene, each with its own reference view.  All device memory.
 *   view [n] i32, ray_idxs [n] i32 (pixel u * H + v), depth [n] f32 (ground-truth distance to the
 *   camera centre), cams [n_views][28] f32 (P_pinv [4][3] | centre [4] | P [3][4], row-major),
 *   nbr [n_views][N] i32 (the views a ray of view v is projected into, nbr[v][0] == v by
 *   convention); H, W, D and the bounding box are the context's.
 * Outputs, every fp32 operation rounded on its own, in this order:
 *   points [n][D][4]      what rn_sample_points gives with cams[view] (bit for bit);
 *   target [n][4]         ray_i = (Pinv_i0 u + Pinv_i1 v) + Pinv_i2, i = 0..3;  a = ray / ray_3 -
 *                         centre;  norm = sqrt((a0^2 + a1^2) + a2^2);  target = a / norm * depth +
 *                         centre, w = 1 (depth taken as 0 for a ray without depth);
 *   centres [n][N][D][2]  i32 (x = column, y = row): q = ((P0 X + P1 Y) + P2 Z) + P3 per row of
 *                         cams[nbr[view][j]].P, x = qx / qz, y = qy / qz, rounded half to even and
 *                         converted (NaN -> 0, beyond int32 -> the nearest end);
 *   flags [n] i32         1 no depth (depth == 0 or not finite) | 2 target not inside the box
 *                         (some coordinate < min, > max or NaN) | 4 the ray misses the box
 *                         (t_near > t_far of the slab test, before its swap) | 8 some patch of
 *                         some view crosses an image border: not (cx - w/2 >= 0, cy - h/2 >= 0,
 *                         cx + w/2 + w%2 <= W, cy + h/2 + h%2 <= H), or x, y not finite, or
 *                         qz <= 0.  A ray is valid iff its flags are 0.
 * A view outside [0, n_views), a ray index outside [0, H W) or such a neighbour is never read
 * through: the kernel tests them, writes zeros and flags = 16 for that ray and the CALL returns
 * RN_ERR_INVALID -- decided on the host from one word the kernel ORs into, so the entry
 * synchronises `stream`.  n == 0: RN_OK, no launch.  n * N * D < 2^30. */
int rn_batch_rays(rn_ctx *ctx, int32_t n, const int32_t *view, const int32_t *ray_idxs,
                  const float *depth, const float *cams, int32_t n_views, const int32_t *nbr,
                  int32_t N, int32_t patch_h, int32_t patch_w, float *points, float *target,
                  int32_t *centres, int32_t *flags, void *stream);

/* The patches around rn_batch_rays' centres.  images [n_views][H][W][C] f32 (channels-last),
 * view [n], centres [n][N][D][2], nbr [n_views][N] as above.  patches [N][n][D][patch_h][patch_w][C]
 * f32: patch j of ray r and sample k holds image nbr[view[r]][j] at rows cy - h/2 .. cy + h/2 +
 * h%2 - 1 and columns cx - w/2 .. cx + w/2 + w%2 - 1, zero wherever that lies outside the image.
 * EVERY texel read is tested against the image: a centre may be any int32.  Index checks, the
 * synchronisation and n == 0 as for rn_batch_rays. */
int rn_batch_patches(rn_ctx *ctx, int32_t n, const float *images, int32_t n_views, int32_t C,
                     const int32_t *view, const int32_t *centres, const int32_t *nbr, int32_t N,
                     int32_t patch_h, int32_t patch_w, float *patches, void *stream);

/* ---- sampling schemes: WHERE on the viewing ray the D samples lie ----
 *
 * The ray of a pixel is what sample_in_bbox computes (sampling_schemes.cu:44-90): pixel (u, v) =
 * (ray_idx / H, ray_idx % H); o_r = fl32(Pinv_r0 u) + fl32(Pinv_r1 v) + Pinv_r2 summed in fp64,
 * r = 0..3; dir_i = fl32(o_i / o_3 - centre_i).  The schemes share it.
 *
 * RN_SAMPLE_IN_BBOX       the box segment of the slab test, sample k = plane_point(s, e, k, D) =
 *                         s + k (e - s) / (D - 1) per coordinate in fp32: the old entries.
 * RN_SAMPLE_IN_RANGE      (raynet/common/sampling_schemes.py:178-237) range = (r0, r1):
 *                         d^ = dir / sqrt((dir0^2 + dir1^2) + dir2^2), s = centre + r0 d^,
 *                         e = centre + r1 d^, sample k = plane_point(s, e, k, D); every fp32
 *                         operation rounded on its own, in this order.  The box plays no part.
 * RN_SAMPLE_IN_DISPARITY  (sampling_schemes.py:240-297) the box segment (p_near, p_far) is
 *                         projected into the far view -- the LAST view of the ray's neighbour
 *                         list --, D pixels lie evenly between the two projections, each is
 *                         back-projected through the far view's P_inv, and sample k is the point
 *                         ON THE VIEWING RAY closest to that ray (utils/geometry.py:243-312, first
 *                         returned point).  In fp64 from the fp32 segment ends on, one rounding
 *                         to fp32 at the end; with a.b = (a0 b0 + a1 b1) + a2 b2:
 *                           q = ((P0 X + P1 Y) + P2 Z) + P3 per row of far_P;
 *                           pix = (rint(qx/qz), rint(qy/qz)), half to even (Image.project rounds)
 *                           t_k = fl32(k * (1 / (D - 1))) (fp64 product), t_{D-1} = 1
 *                           pu = fl32(u_near + t_k (u_far - u_near)), pv likewise (Image.ray
 *                           takes a float32 pixel)
 *                           o_r = (Pinv_r0 pu + Pinv_r1 pv) + Pinv_r2;  a2 = o / o_3 - c2
 *                           a1 = dir, c1 = centre, c2 = far_centre
 *                           div = (a1.a1)(a2.a2) - (a1.a2)(a1.a2)
 *                           t1 = (-(a2.a2) (a1.c1 - a1.c2) + (a1.a2) (a2.c1 - a2.c2)) / div
 *                           point = fl32(c1 + a1 t1)
 *                         A ray that misses the box (t_near > t_far; the reference returns None)
 *                         has no samples: its D points are the camera centre with w = 0, its
 *                         K9 column the sweep of that one point (1 / D each), its K10 depth 0.
 *                         Every other point has w = 1.
 * The POD is host memory, read during the call.  The far view is used by RN_SAMPLE_IN_DISPARITY
 * only, the range by RN_SAMPLE_IN_RANGE only. */
typedef enum {
    RN_SAMPLE_IN_BBOX = 0,
    RN_SAMPLE_IN_RANGE = 1,
    RN_SAMPLE_IN_DISPARITY = 2
} rn_sampling_scheme;

typedef struct {
    int32_t scheme;          /* rn_sampling_scheme */
    float range[2];          /* r0 < r1, both finite and > 0 */
    float far_P[12];         /* [3][4] row-major */
    float far_P_inv[12];     /* [4][3] row-major */
    float far_centre[4];
} rn_sampling;

/* Every entry below: `sampling` NULL, an unknown scheme, a range that is not 0 < r0 < r1 <
 * infinity (RN_SAMPLE_IN_RANGE) or D < 2 is RN_ERR_INVALID with a message in rn_last_error and
 * no launch (D < 2 is refused by rn_create already, which has no context to leave a message in:
 * the entries' own check guards a context made some other way); n == 0 is RN_OK without a launch; RN_SAMPLE_IN_BBOX runs the old entry's kernel
 * (same bits).  RN_SAMPLE_IN_RANGE sweeps run the old entries' kernels on the range segments
 * (the context keeps ONE buffer of segments: per context, issue them on one stream at a time);
 * RN_SAMPLE_IN_DISPARITY sweeps take one ray per wavefront, also where D <= 32 packs two or four
 * bbox rays into one. */

/* K8 under a scheme (sampling_schemes.py:183-195, :241-297; sample_points.py:12-54):
 * points [n][D][4] */
int rn_sample_points_scheme(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *P_inv,
                            const float *camera_center, const rn_sampling *sampling,
                            float *points, void *stream);

/* K9 under a scheme (similarities.py:101-130 with scripts/forward_pass.py:91's scheme): S [n][D] */
int rn_mvcnn_similarities_scheme(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs,
                                 const float *features, const float *P, const float *P_inv,
                                 const float *camera_center, const rn_sampling *sampling,
                                 float *S, void *stream);

/* K10 under a scheme (similarities.py:252-285): points are rn_sample_points_scheme's bit for
 * bit, the plane is the first maximum of the column, depth_map its point's distance to the
 * camera centre */
int rn_mvcnn_depth_scheme(rn_ctx *ctx, int32_t n, const int32_t *ray_idxs, const float *features,
                          const float *P, const float *P_inv, const float *camera_center,
                          const rn_sampling *sampling, float *S, float *points,
                          float *depth_map, void *stream);

/* rn_batch_rays under a scheme (pretrain_network.py:191's sample generators): points are what
 * rn_sample_points_scheme gives with cams[view] and, for RN_SAMPLE_IN_DISPARITY, the far view
 * cams[nbr[view][N - 1]] (the POD's far view is not read); target, centres and flags follow
 * rn_batch_rays' definitions on those points.  Flag 4 is never set by RN_SAMPLE_IN_RANGE. */
int rn_batch_rays_scheme(rn_ctx *ctx, int32_t n, const int32_t *view, const int32_t *ray_idxs,
                         const float *depth, const float *cams, int32_t n_views,
                         const int32_t *nbr, int32_t N, int32_t patch_h, int32_t patch_w,
                         const rn_sampling *sampling, float *points, float *target,
                         int32_t *centres, int32_t *flags, void *stream);

/* ---- the occupancy volume: what the MRF believes about every voxel ----
 *
 * belief_out [gx][gy][gz] f32: belief = occupancy_to_ray(bias + acc[voxel], 0), the occupancy
 * k_bp / k_depth read for a voxel whose ray sends no message -- the same device function, the
 * clamp to [1e-4, fl32(1 - 1e-4)] included.  acc: bricked != 0, the resident path's 4x4x4-bricked
 * buffer of rn_acc_size() floats (the padding voxels of partial bricks are never read); bricked
 * == 0, the [gx][gy][gz] array.  bias: the prior where the accumulator holds the sums of the
 * messages only (the plan path without fixed-point sums), else 0.  One pass over the grid.  A NULL
 * pointer or a `bricked` other than 0 / 1 is RN_ERR_INVALID, no launch. */
int rn_occupancy_grid(rn_ctx *ctx, const float *acc, int32_t bricked, float bias,
                      float *belief_out, void *stream);

/* A belief grid seen along n ray segments.  ray_start / ray_end [n][3] as rn_sample_rays and the
 * scheme entries write them; belief [gx][gy][gz] f32 with values in [0, 1] (rn_occupancy_grid's);
 * camera_center [3].  The voxels v_0 .. v_{c-1} of a ray are the list rn_voxel_traversal emits for
 * its segment in this context (same DDA, capped at the context's M; never written to memory).
 * In fp32, every operation rounded on its own, in this order:
 *     o_i = belief[v_i];  T_0 = 1;  w_i = o_i T_i;  T_{i+1} = T_i (1 - o_i)
 *     t_i = sqrt(((x - cx)^2 + (y - cy)^2) + (z - cz)^2), (x, y, z) the centre of v_i
 *           (rn_set_voxel_grid's axis tables): the depth arithmetic of rn_scene_depth
 *     i*  = the first i whose w_i is greater than every earlier w (strictly; i = 0 qualifies)
 * out[plane * out_stride + ray], out_stride >= n, nothing written at or beyond a plane's n-th
 * entry:
 *     0 depth           t_{i*}
 *     1 opacity         1 - T_c
 *     2 expected depth  (sum_i w_i t_i) / (sum_i w_i), both sums in list order from 0, one IEEE
 *                       division (0 where sum_i w_i is not positive)
 *     3 confidence      w_{i*}
 *     4 median depth    t_i of the first i with T_{i+1} <= 0.5, 0 where no i has
 * A ray with c = 0 (it misses the box, or its first cell lies outside the grid) has 0 in every
 * plane.  n == 0: RN_OK, no launch.  n < 0, a NULL pointer or out_stride < n: RN_ERR_INVALID,
 * no launch.  rn_set_voxel_grid must have been called (RN_ERR_STATE). */
int rn_volume_render(rn_ctx *ctx, int32_t n, const float *ray_start, const float *ray_end,
                     const float *camera_center, const float *belief, float *out,
                     int64_t out_stride, void *stream);

/* ---- the surface of a belief grid: an indexed triangle mesh ----
 *
 * Marching tetrahedra over the Kuhn split of every lattice cell.  belief [gx][gy][gz] f32, finite;
 * iso f32; closed 0 / 1; the context's axis tables (rn_set_voxel_grid, else RN_ERR_STATE).
 *
 * Lattice: the points (i, j, k), i in [-c, gx - 1 + c] with c = closed, likewise j and k: n = g + 2c
 * per axis, x slowest and z fastest in the linear order, value 0 outside the grid.  Its cells are
 * the cubes at the base points (all three coordinates below n - 1), in the base points' order.  A
 * lattice with an axis of a single point has no cells and its mesh is empty, vertices included.
 * Coordinates: on axis a the table entry A[i] inside the grid, A[-1] = fl(A[0] - h) and
 * A[g] = fl(A[g - 1] + h) with h = fl(fl(bbox[3 + a] - bbox[a]) / g).
 * inside(p) = value(p) >= iso (the side volume.OccupancyVolume.pointcloud takes; NaN is outside).
 * Edges: (p, d), d in 1..7 (bit 0: +x, bit 1: +y, bit 2: +z) with q = p + d in the lattice; an
 * edge carries a vertex iff inside(p) != inside(q).  Vertices are ordered by p, then by d.  With
 * a = value(p), b = value(q), in fp32, every operation rounded on its own, the division IEEE:
 *     t = (iso - a) / (b - a)
 *     coordinate = A[p]                             on an axis d does not move along
 *                  A[p] + t * (A[q] - A[p])         on the others -- always from p to q
 * Tetrahedra of a cell, as corner masks relative to its base point, in this order:
 *     [0,1,3,7] [0,1,5,7] [0,2,3,7] [0,2,6,7] [0,4,5,7] [0,4,6,7]
 * with local corners 0..3 in that order.  Triangles of a tetrahedron, as the edges their corners
 * lie on:
 *     one inside corner a, outside o1 < o2 < o3:      (a o1, a o2, a o3)
 *     three inside i1 < i2 < i3, outside o:           (i1 o, i2 o, i3 o)
 *     two inside a < b, outside c < d:                (ac, ad, bd) then (ac, bd, bc)
 * and the last two entries swapped where the right-hand normal would else point from outside to
 * inside (a constant per tetrahedron and case).  Triangles are ordered by cell, then tetrahedron,
 * then as above; an entry is the index of the vertex on its edge (base point of the lower mask,
 * higher mask XOR lower mask).  With closed = 1 the surface is a closed, consistently oriented
 * 2-manifold for every input (triangles at values equal to iso may have no area); with closed = 0
 * it is open where it meets the lattice's hull.  The arrays are the same whatever the launch
 * geometry.
 *
 * rn_isosurface_workspace_bytes: the bytes both entries need at `workspace` (8-byte aligned), -1
 * for a bad argument or a lattice of L points with 12 L >= 2^31.
 * rn_isosurface_count: classifies every point, scans the counts over the whole lattice and
 * returns totals_host[0] = nv, totals_host[1] = nf ON THE HOST: it synchronises `stream` and so
 * cannot be captured into a graph.  A lattice without cells: both 0, no launch.
 * rn_isosurface_emit: after a count of the same belief, iso, closed and workspace, with its
 * totals: writes vertices_out [nv][3] f32 and faces_out [nf][3] i32, exactly nv and nf rows (rows
 * at or beyond nv / nf are never written, whatever the workspace holds).  nv == nf == 0: RN_OK, no
 * launch.
 * RN_ERR_INVALID, rn_last_error naming the entry, no launch: a NULL pointer, closed not 0 / 1, a
 * non-finite iso, iso <= 0 with closed (the padding's 0 must be outside), 12 L >= 2^31, a
 * workspace that is not 8-byte aligned, nv / nf negative or beyond 7 L / 12 cells.
 * A non-finite belief may give non-finite positions; it never causes a write out of range: the
 * counts and every index depend on the comparisons value >= iso only. */
int64_t rn_isosurface_workspace_bytes(rn_ctx *ctx, int32_t closed);
int rn_isosurface_count(rn_ctx *ctx, const float *belief, float iso, int32_t closed,
                        void *workspace, int64_t *totals_host, void *stream);
int rn_isosurface_emit(rn_ctx *ctx, const float *belief, float iso, int32_t closed,
                       const void *workspace, int64_t nv, int64_t nf, float *vertices_out,
                       int32_t *faces_out, void *stream);

/* ---- what a surface looks like: vertex normals and colours from the images ----
 *
 * All arrays are device memory.  Every floating-point operation below is fp64 and rounded on its
 * own, in the order written (the library is built with -ffp-contract=off); only + - * /, floor,
 * rint, comparisons and conversions occur -- no sqrt -- so a NumPy restatement gives the same bits
 * (tests/appearance_truth.py).
 *
 * rn_vertex_area_normals: vertices [nv][3] f32, faces [nf][3] i32, the corner table of the mesh
 * by vertex -- corners [3 nf] i32: the indices c = 3 face + slot of the flattened `faces`, sorted
 * by the vertex they name, ascending c within a vertex; offsets [nv + 1] i32: the exclusive prefix
 * of the vertices' corner counts -- and normals [nv][3] f32, written.  One thread per vertex v,
 * over k = offsets[v] .. offsets[v + 1] - 1 in that order:
 *     f = corners[k] / 3;  p0, p1, p2 = the vertices of faces[f];  e1 = p1 - p0;  e2 = p2 - p0
 *     a = (e1.y e2.z - e1.z e2.y,  e1.z e2.x - e1.x e2.z,  e1.x e2.y - e1.y e2.x);  s = s + a
 * and normals[v] = (float) s: area-weighted, NOT normalised (its length is twice the area around
 * the vertex); (0, 0, 0) for a vertex in no face.  A k outside [0, 3 nf), a corner outside
 * [0, 3 nf) and a face with a vertex index outside [0, nv) are skipped: whatever the three index
 * arrays hold, nothing is read or written out of bounds.  nv == 0: RN_OK, no launch.
 * RN_ERR_INVALID, rn_last_error naming the entry, no launch: nv or nf negative, nv > 2^31 - 2,
 * 3 nf > 2^31 - 1, a NULL vertices / offsets / normals, a NULL faces / corners with nf > 0.
 *
 * rn_project_colors: points [n][3] f32; normals [n][3] f32 or NULL; cameras [V][15] f64, a row
 * P [3][4] row-major | centre [3]; images [V][H][W][C] f32; depths [V][H][W] f32 or NULL,
 * distances to the camera centre; pixel centres at whole coordinates (both as rn_depthmap_points
 * and rn_consistency_tau have them).  1 <= C <= 4, 0 <= V <= 32.  Written: colors [n][C] f32,
 * weight [n] f32, views [n] u32 -- all n rows, always, also with V == 0.  One thread per point
 * p = (x, y, z) with normal n, the views v in ascending order:
 *   projection  h_k = ((P_k0 x + P_k1 y) + P_k2 z) + P_k3;  X = h_0 / h_2;  Y = h_1 / h_2
 *               d = c - p;  dd = (d_x^2 + d_y^2) + d_z^2
 *   in view     0 < h_2 < inf,  dd > 0,  border <= X <= (W - 1) - border,
 *               border <= Y <= (H - 1) - border          (a NaN fails every test)
 *   facing      with normals and nn = (n_x^2 + n_y^2) + n_z^2 > 0:
 *                   dot = (n_x d_x + n_y d_y) + n_z d_z;  q = nn dd
 *                   the view counts only if dot > 0 and dot dot > (min_cos min_cos) q
 *                   w = (dot dot) / q                     (cos^2)
 *               else w = 1 and there is no facing test
 *   occlusion   with depths: z = depths[v][rint(Y)][rint(X)] (half to even);  lim = z + tol
 *               the view counts only if z > 0 and dd <= lim lim  -- one-sided: a point in front
 *               of the recorded surface is seen; z = +inf occludes nothing; 0, a negative value
 *               or NaN hides the point
 *   colour      x0 = floor(X);  x1 = min(x0 + 1, W - 1);  fx = X - x0;  likewise y
 *               top = I00 + fx (I01 - I00);  bot = I10 + fx (I11 - I10);  col = top + fy (bot - top)
 *   combination mode 0 (blend): num_c = num_c + w col_c;  den = den + w;  colors = (float)(num_c / den)
 *               mode 1 (best):  colors = (float) col of the first view with the largest w
 *               weight = (float) den in both modes;  bit v of views is set iff view v counted
 * A point no view counts for has colour 0, weight 0 and views 0.  A view that does not count
 * reads pixel (0, 0) of its image and depth map, so every load lies inside the arrays whatever the
 * point.  n == 0: RN_OK, no launch.  RN_ERR_INVALID, rn_last_error naming the entry, no launch: n
 * negative, n C > 2^31 - 1, V outside 0..32, C outside 1..4, H or W below 1, tol negative or not
 * finite, min_cos outside [0, 1), border negative or not finite, mode outside {0, 1}, a NULL
 * points / colors / weight / views, a NULL cameras / images with V > 0. */
int rn_vertex_area_normals(rn_ctx *ctx, int64_t nv, const float *vertices, int64_t nf,
                           const int32_t *faces, const int32_t *offsets, const int32_t *corners,
                           float *normals, void *stream);
int rn_project_colors(rn_ctx *ctx, int64_t n, const float *points, const float *normals,
                      int32_t V, const double *cameras, int32_t H, int32_t W, int32_t C,
                      const float *images, const float *depths, double tol, double min_cos,
                      double border, int32_t mode, float *colors, float *weight, uint32_t *views,
                      void *stream);

/* ---- depth maps fused into a truncated signed distance volume ----
 *
 * rn_tsdf_integrate: every view into the context's grid in one launch.  All arrays are device
 * memory.  cameras [V][15] f64, a row P [3][4] row-major | centre [3] (as for rn_project_colors);
 * depths [V][H][W] f32, distances to the camera centre, pixel centres at whole coordinates;
 * weights [V][H][W] f32 or NULL for weight 1.  0 <= V <= 4096 (the bound rejects garbage; it is no
 * capacity).  Written: tsdf [gx][gy][gz] f32 and weight [gx][gy][gz] f32 over the context's grid --
 * all G entries, always, also with V == 0; both are finite whatever the inputs hold.
 *
 * One thread per voxel; its centre p = (x, y, z) is the context's axis tables (rn_set_voxel_grid)
 * converted to double; the views v in ascending order.  Every operation is fp64 and rounded on its
 * own, in the order written (the library is built with -ffp-contract=off); only + - * /, rint, min,
 * comparisons and conversions occur -- no sqrt -- so a NumPy restatement gives the same bits
 * (tests/fusion_truth.py):
 *   projection   h_k = ((P_k0 x + P_k1 y) + P_k2 z) + P_k3;  X = h_0 / h_2;  Y = h_1 / h_2
 *                d = c - p;  dd = (d_x^2 + d_y^2) + d_z^2    (exactly as rn_project_colors)
 *   in view      0 < h_2 < inf,  dd > 0,  border <= X <= (W - 1) - border,
 *                border <= Y <= (H - 1) - border             (a NaN fails every test)
 *   measurement  z = depths[v][rint(Y)][rint(X)] (half to even); counts only if 0 < z < inf
 *                (0, a negative value, NaN and +inf are "no measurement")
 *   weight       w = 1, or w = weights[v][the same pixel]; counts only if 0 < w < inf
 *   distance     s = (z z - dd) / (z + z)
 *   behind       the view counts only if s >= -trunc
 *   value        t = min(s / trunc, 1)
 *   sums         num = num + w t;  den = den + w
 *   result       den > 0:  tsdf = (float)(num / den),  weight = (float) den
 *                else:     tsdf = 1.0f,                weight = 0.0f
 * A view that does not count reads pixel (0, 0) of its maps, so every load lies inside the arrays
 * whatever the cameras hold.
 *
 * s is (z - r)(z + r) / 2z with r = sqrt(dd), the distance of the voxel from the camera: it is 0
 * exactly where r = z and monotone in r, so its zero crossing -- all the surface depends on -- is
 * the true one; it differs from z - r by the factor 1 - (z - r) / 2z, inside the band at most
 * trunc / 2z; and it needs no sqrt, which is what lets a restatement give the same bits.  tsdf > 0
 * in front of the surface (free space, 1 at trunc and beyond), < 0 behind it down to -1; a voxel
 * more than trunc behind every surface it is seen against is unobserved by that view.
 *
 * RN_ERR_INVALID, rn_last_error naming the entry, no launch: V outside 0..4096, H or W below 1,
 * trunc not finite or <= 0, border negative or not finite, a NULL tsdf or weight, a NULL cameras or
 * depths with V > 0.  RN_ERR_STATE before rn_set_voxel_grid. */
int rn_tsdf_integrate(rn_ctx *ctx, int32_t V, const double *cameras, int32_t H, int32_t W,
                      const float *depths, const float *weights, double trunc, double border,
                      float *tsdf, float *weight, void *stream);

/* ---- what the other views say about a point ----
 *
 * rn_points_consistency: every view's verdict on every point in one launch.  All arrays are device
 * memory.  points [3][n] f64, the coordinates as three rows (the layout rn_depthmap_points writes);
 * cameras [V][15] f64, a row P [3][4] row-major | centre [3] (as for rn_project_colors); depths
 * [V][H][W] f32, distances to the camera centre, pixel centres at whole coordinates.
 * 1 <= V <= 32; exclude: the one view that is skipped (the view the points came from), -1 for
 * none.  Written: seen, agree, violate [n] u32, bit v for view v, and residual [n] f32 -- all n
 * entries, always.
 *
 * One thread per point p = (x, y, z); the views v in ascending order, v == exclude skipped.  Every
 * operation is fp64 and rounded on its own, in the order written (the library is built with
 * -ffp-contract=off); only + - * /, rint, comparisons and conversions occur -- no sqrt -- so a
 * NumPy restatement gives the same bits (tests/consistency_truth.py):
 *   projection   exactly as rn_project_colors and rn_tsdf_integrate: X, Y, dd, and
 *   in view      0 < h_2 < inf,  dd > 0,  border <= X <= (W - 1) - border,
 *                border <= Y <= (H - 1) - border             (a NaN fails every test)
 *   measurement  z = depths[v][rint(Y)][rint(X)] (half to even);
 *                measured = in view and 0 < z < inf
 *   distance     s = (z z - dd) / (z + z);   t = tol_abs + tol_rel z
 *   verdict      agrees   = measured and -t <= s <= t
 *                violates = measured and s > t      (the view sees past the point: the point
 *                                                    floats in that view's free space)
 *                a measured view with s < -t only fails to see the point (it is occluded there):
 *                bit v of seen alone
 *   masks        bit v of seen / agree / violate is set iff measured / agrees / violates
 *   sums         where the view agrees: num = num + s;  cnt = cnt + 1
 *   result       residual = cnt > 0 ? (float)(num / cnt) : 0.0f
 * A view that is not in view reads pixel (0, 0) of its map, so every load lies inside the arrays
 * whatever the points and cameras hold.  A NaN or infinite point sets no bit.  The depth is read at
 * the nearest pixel: a tolerance must exceed the depth step of one pixel of the surfaces it is to
 * confirm.
 *
 * n == 0: RN_OK, no launch.  RN_ERR_INVALID, rn_last_error naming the entry, no launch: n negative
 * or above 2^38, V outside 1..32, H or W below 1, exclude outside -1..V-1, tol_abs, tol_rel or
 * border negative or not finite, and with n > 0 a NULL points, cameras, depths, seen, agree,
 * violate or residual. */
int rn_points_consistency(rn_ctx *ctx, int64_t n, const double *points, int32_t V,
                          const double *cameras, int32_t H, int32_t W, const float *depths,
                          int32_t exclude, double tol_abs, double tol_rel, double border,
                          uint32_t *seen, uint32_t *agree, uint32_t *violate, float *residual,
                          void *stream);

/* ---- which views to use: shared visibility, pair counts, covering sets ----
 *
 * rn_view_overlap: which of up to 64 views see every point, and how many points every pair of
 * views shares at a useful triangulation angle.  All arrays are device memory.  points [3][n] f64,
 * the coordinates as three rows; normals [3][n] f64 or NULL (no facing test); cameras [V][15] f64,
 * a row P [3][4] row-major | centre [3] (as for rn_project_colors); depths [V][H][W] f32, distances
 * to the camera centre, or NULL (no occlusion test).  1 <= V <= 64.  0 <= cos_lo <= cos_hi <= 1 are
 * COSINES of the largest and the smallest triangulation angle that counts.
 *
 * Every operation is fp64 and rounded on its own, in the order written (the library is built with
 * -ffp-contract=off); only + - * /, rint, comparisons and conversions occur -- no sqrt, no libm --
 * and every count is an integer added by integer atomics, so the result is one fixed array
 * whatever order the hardware ran the threads in, and a NumPy restatement gives the same integers
 * (tests/view_selection_truth.py).
 *
 * View v sees point p = (x, y, z) with normal m -- exactly the per-view test of rn_project_colors,
 * without the colour fetch:
 *   projection   X, Y, d = c_v - p, dd = (d_x^2 + d_y^2) + d_z^2 and
 *   in view      0 < h_2 < inf,  dd > 0,  border <= X <= (W - 1) - border,
 *                border <= Y <= (H - 1) - border             (a NaN fails every test)
 *   facing       with nn = (m_x^2 + m_y^2) + m_z^2 > 0 only:  dot = (m_x d_x + m_y d_y) + m_z d_z;
 *                dot > 0  and  dot dot > (min_cos min_cos) (nn dd)
 *   occlusion    with depths only:  zf = depths[v][rint(Y)][rint(X)] (half to even; a view that
 *                does not count so far reads pixel (0, 0));  zf > 0  and  dd <= (zf + tol)^2
 * Views i < j share p when both see it and, with a = c_i - p, b = c_j - p, dd_i, dd_j as above,
 *   dot = (a_x b_x + a_y b_y) + a_z b_z;   q = dd_i dd_j;   dot2 = dot dot
 *   dot > 0  and  dot2 >= lo2 q  and  dot2 <= hi2 q,   lo2 = cos_lo cos_lo,  hi2 = cos_hi cos_hi
 * The band is decided on the squares as computed: with centres (0, 0, 4) and (3, 0, 4) and the
 * point at the origin the cosine is 4/5 in exact arithmetic, but 0.8 * 0.8 * 400 rounds to
 * 256.00000000000006 > 256 = dot2, and the pair does not count at cos_lo = 0.8.
 *
 * Written: visible [n] u64, bit v set iff view v sees point p, bits V and above 0 -- all n
 * entries, always.  pairs [V][V] i64 is ADDED to: pairs[i][i] += the number of points view i sees,
 * pairs[i][j] += the number of points i and j share for i < j; the lower triangle is never touched.
 * The caller zeroes pairs; integer sums are free of order, so calls over the parts of a cloud add
 * up to exactly the call over the whole.  A NaN or infinite point sets no bit.
 *
 * n == 0: RN_OK, no launch.  RN_ERR_INVALID, rn_last_error naming the entry, no launch: n negative
 * or above 2^38, V outside 1..64, H or W below 1, tol, min_cos or border negative or not finite,
 * cos_lo, cos_hi not 0 <= cos_lo <= cos_hi <= 1, and with n > 0 a NULL points, cameras, visible or
 * pairs. */
int rn_view_overlap(rn_ctx *ctx, int64_t n, const double *points, const double *normals,
                    int32_t V, const double *cameras, int32_t H, int32_t W, const float *depths,
                    double tol, double min_cos, double border, double cos_lo, double cos_hi,
                    uint64_t *visible, int64_t *pairs, void *stream);

/* rn_view_gain: one round of a greedy covering set over rn_view_overlap's masks.  visible [n] u64
 * and gain [V + 1] i64 are device memory; chosen is a 64-bit mask of the views taken so far, passed
 * as a bit pattern (bit 63 is the sign bit).  A point is short when
 *   popcount(visible[p] & chosen & (the low V bits)) < redundancy.
 * gain is ADDED to: gain[v] += the number of short points with bit v set, for every v < V that is
 * not in chosen (the entries of chosen views are not touched), and gain[V] += the number of short
 * points.  The caller zeroes gain.  1 <= V <= 64, 1 <= redundancy <= 64.
 *
 * n == 0: RN_OK, no launch.  RN_ERR_INVALID, rn_last_error naming the entry, no launch: n negative
 * or above 2^38, V or redundancy outside 1..64, and with n > 0 a NULL visible or gain. */
int rn_view_gain(rn_ctx *ctx, int64_t n, const uint64_t *visible, int32_t V, int64_t chosen,
                 int32_t redundancy, int64_t *gain, void *stream);

/* ---- the connected components of an indexed triangle mesh ----
 *
 * rn_mesh_components: which piece every vertex belongs to, and how large the pieces are.  Two
 * vertices are connected if a face names both; a component is a class of the transitive closure.
 * Positions play no part, and the entry does not take them: two pieces that touch only in space,
 * with duplicated vertex rows, are two components.  (The marching-tetrahedra meshes of
 * rn_isosurface_emit share one vertex per lattice edge, so for them "connected" is what one
 * expects.)
 *
 * All arrays are device memory.  faces [nf][3] i32; labels, vertex_counts and face_counts [nv] i32,
 * written in all nv entries, always; status [1] i32.  vertex_counts, face_counts and status may
 * each be NULL: not wanted.
 *   labels[v]         the smallest vertex index of v's component; a vertex in no face is its own
 *                     component.  Hence labels[v] <= v and labels[labels[v]] == labels[v], and the
 *                     result is one fixed array whatever the launch geometry or the order in which
 *                     the hardware ran the threads.
 *   vertex_counts[r]  the number of vertices with label r
 *   face_counts[r]    the number of counted faces whose first vertex has label r
 * Both counts are 0 at every r that is not a label; they are integers added by integer atomics,
 * so they are exact.
 *
 * A face with any index outside [0, nv) is skipped as a whole: it connects nothing and is counted
 * nowhere; whatever `faces` holds, nothing is read or written out of bounds.  Degenerate faces
 * count like any other: (a, a, b) connects a and b, (a, a, a) connects nothing; duplicate faces
 * count once each.
 *
 * status[0] is 0 after every correct run, 1 if a pointer chase of the union-find reached its bound
 * of nv + 1 steps -- which cannot happen while parent[x] <= x holds; it exists so
 * that a bug ends as an error and not as a hang.
 *
 * nv == 0: RN_OK, no launch.  RN_ERR_INVALID, rn_last_error naming the entry, no launch, outputs
 * untouched: nv or nf negative, nv > 2^31 - 2, 3 nf > 2^31 - 1, a NULL labels, a NULL faces with
 * nf > 0. */
int rn_mesh_components(rn_ctx *ctx, int64_t nv, int64_t nf, const int32_t *faces,
                       int32_t *labels, int32_t *vertex_counts, int32_t *face_counts,
                       int32_t *status, void *stream);

/* ---- Taubin smoothing of an indexed triangle mesh ----
 *
 * rn_mesh_smooth: the vertices of a mesh moved towards the mean of their neighbours and back
 * (Taubin's lambda | mu scheme), so that the terraces of an iso-surface and the noise of a fused
 * one flatten while the surface keeps its size.  The faces do not change.
 *
 * All arrays are device memory.  vertices_in and vertices_out [nv][3] f32; faces [nf][3] i32;
 * offsets [nv + 1] i32 and corners [3 nf] i32: the corner table of rn_vertex_area_normals; fixed
 * [nv] u8 or NULL: a non-zero entry pins that vertex; workspace: 8-byte aligned, at least
 * rn_mesh_smooth_workspace_bytes(ctx, nv, nf) bytes (-1 for sizes rn_mesh_smooth refuses), laid
 * out ring [3 nf][2] i32 | scratch [nv][3] f32.  Nothing beyond that size is touched.
 *
 * The ring, written once per call, one thread per table position k in [0, 3 nf):
 *     c = corners[k];  f = c / 3;  slot = c % 3
 *     ring[2k] = faces[f][(slot + 1) % 3];  ring[2k + 1] = faces[f][(slot + 2) % 3]
 * both -1 instead if c is outside [0, 3 nf) or any of the face's three indices is outside [0, nv).
 *
 * One step with factor t from src to dst, one thread per vertex v.  Every operation is fp64 and
 * rounded on its own, in the order written (the library is built with -ffp-contract=off); only
 * + - * /, comparisons and conversions occur, so a NumPy restatement gives the same bits
 * (tests/smooth_truth.py):
 *     p = (double) src[v];  s = 0;  m = 0
 *     for k = offsets[v] .. offsets[v + 1] - 1, the range cut to [0, 3 nf), ascending:
 *         a = ring[2k];  b = ring[2k + 1];  if a < 0: continue
 *         s = (s + (double) src[a]) + (double) src[b]          per coordinate
 *         m = m + 2
 *     if m == 0 or (fixed and fixed[v]):  dst[v] = src[v]      (the bits)
 *     else:  x = p + t * (s / (double) m - p)                  per coordinate
 *            lo = (double) in[v] - max_move;  hi = (double) in[v] + max_move
 *            if x < lo: x = lo;   if x > hi: x = hi            (a NaN passes both tests)
 *            dst[v] = (float) x
 * Every incident triangle gives its two other vertices: on a closed manifold mesh each neighbour
 * appears in two triangles and this is the uniform umbrella operator; at an open border the border
 * neighbours weigh half, which is what `fixed` is for.
 *
 * An iteration is a step with lambda, then a step with mu if mu != 0 (mu == 0: plain Laplacian
 * smoothing): L = iterations * (mu != 0 ? 2 : 1) launches that ping-pong between the scratch and
 * vertices_out, the parity such that step L writes vertices_out.  Positions are f32 between steps.
 * vertices_in is never written and the clamp always refers to it: no coordinate of any vertex ends
 * farther than max_move from where it started; +inf: no clamp.  iterations == 0 copies vertices_in
 * to vertices_out and launches nothing.  No step reads a buffer that another thread of the same
 * launch writes, so the result is one fixed array whatever the order the hardware ran the threads
 * in.
 *
 * Whatever the three index arrays hold, nothing is read or written out of bounds, and no index
 * depends on a floating-point value.  A non-finite position spreads to its neighbours and nowhere
 * else; callers clean first (SurfaceMesh.without_nonfinite).
 *
 * nv == 0: RN_OK, no launch.  RN_ERR_INVALID, rn_last_error naming the entry, no launch, outputs
 * untouched: nv or nf negative, nv > 2^31 - 2, 3 nf > 2^31 - 1, iterations outside 0..10000,
 * lambda not finite or outside (0, 1], mu not finite or outside [-1, 0], max_move NaN or <= 0, a
 * NULL vertices_in / offsets / vertices_out / workspace, a NULL faces / corners with nf > 0, a
 * workspace that is not 8-byte aligned, vertices_out == vertices_in, either of them equal to
 * workspace. */
int64_t rn_mesh_smooth_workspace_bytes(rn_ctx *ctx, int64_t nv, int64_t nf);
int rn_mesh_smooth(rn_ctx *ctx, int64_t nv, const float *vertices_in, int64_t nf,
                   const int32_t *faces, const int32_t *offsets, const int32_t *corners,
                   const uint8_t *fixed, int32_t iterations, double lambda, double mu,
                   double max_move, void *workspace, float *vertices_out, void *stream);

/* ---- vertex clustering of an indexed triangle mesh on a uniform grid ----
 *
 * rn_mesh_simplify: the vertices of a mesh that share a cell of a uniform grid become one vertex at
 * their mean; faces that lose a corner that way vanish, vertices no face is left for vanish with
 * them (Rossignac and Borrel's vertex clustering).
 *
 * origin [3] f64, cell [3] f64 and dims [3] i32 are HOST arrays: the grid's corner, the sides of a
 * cell and the number of cells per axis.  All other arrays are device memory.  vertices_in [nv][3]
 * f32 and faces_in [nf][3] i32 are never written.  The caller allocates the upper bounds:
 *   vertices_out [nv][3] f32   the output vertices
 *   faces_out    [nf][3] i32   the output faces, of output indices
 *   source       [nv]    i32   the smallest input index of each output vertex's cluster
 *   cluster      [nv]    i32   the output index of each input vertex's cluster, -1 if unused
 *   counts       [2]     i64   nv_out, nf_out
 * Only the first nv_out rows of vertices_out and source and the first nf_out rows of faces_out are
 * written, and all nv entries of cluster; the rest keep their bits.  source and cluster may each be
 * NULL: not wanted.  workspace: 8-byte aligned, at least rn_mesh_simplify_workspace_bytes(nv, nf,
 * dims) bytes (-1 for sizes or dims rn_mesh_simplify refuses), laid out table [cells][4] u64 (S_x,
 * S_y, S_z, rep i32 | n i32: 32 bytes per cell) | fscan [nf] u64 | vscan [nv] u64 | the scan's
 * scratch | cell_of [nv] i32.  Nothing beyond that size is touched.
 *
 * Every floating-point operation is fp64 and rounded on its own, in the order written (the library
 * is built with -ffp-contract=off); only + - * /, floor, rint (to nearest, ties to even),
 * comparisons and conversions occur, so a NumPy restatement gives the same bits
 * (tests/simplify_truth.py).
 *
 * The cell of a vertex p, per axis k:
 *     t = ((double) p_k - origin_k) / cell_k;  q_k = floor(t);  u_k = t - q_k   (exact)
 *     w_k = (uint64) rint(u_k * 2097152.0)                                       0 <= w_k <= 2^21
 * The vertex is BINNED if 0 <= q_k < dims_k on all three axes (which a NaN or infinite t fails),
 * into cell (q_x dims_y + q_y) dims_z + q_z.  Any other vertex -- NaN, infinite, outside the grid
 * -- is a SINGLETON: a cluster of its own.
 *
 * Per cell, by integer atomics only: rep = the smallest binned vertex index, n = the number of
 * binned vertices, S_k = the sum of their w_k as u64.  With nv <= 2^31 - 2, S_k < 2^53 and
 * (double) S_k is exact.
 *
 * The position of a cluster: the member's three f32 bits if n == 1 or the cluster is a singleton;
 * otherwise, per axis,
 *     x_k = origin_k + cell_k * ((double) q_k + ((double) S_k / (double) n) / 2097152.0)
 * stored as (float) x_k.
 *
 * A face maps each of its indices to the cluster of that vertex, named by rep, or by the vertex
 * itself for a singleton.  It is KEPT if all three indices lie in [0, nv) and the three clusters
 * are pairwise different; kept faces keep their order and their winding.  A cluster is USED if a
 * kept face names it; the used clusters are the output vertices, in ascending order of `source`,
 * so no output vertex is in no face.
 *
 * The result is one fixed set of arrays whatever the launch geometry or the order in which the
 * hardware ran the threads.  Whatever the face indices and the positions hold, nothing is read or
 * written out of bounds, and no loop has a trip count that depends on data.
 *
 * nv == 0: RN_OK, counts = {0, 0}, no kernel launch.  RN_ERR_INVALID, rn_last_error naming the
 * entry, no launch, outputs untouched: nv or nf negative, nv > 2^31 - 2, 3 nf > 2^31 - 1, a dims_k
 * < 1, dims_x dims_y dims_z > 2^31 - 1, a cell_k not finite or <= 0, an origin_k not finite, a NULL
 * origin / cell / dims / counts, and with nv > 0 a NULL vertices_in / vertices_out / workspace, a
 * NULL faces_in / faces_out with nf > 0, a workspace that is not 8-byte aligned, vertices_out ==
 * vertices_in, faces_out == faces_in, either output equal to workspace. */
int64_t rn_mesh_simplify_workspace_bytes(int64_t nv, int64_t nf, const int32_t dims[3]);
int rn_mesh_simplify(rn_ctx *ctx, int64_t nv, const float *vertices_in, int64_t nf,
                     const int32_t *faces_in, const double origin[3], const double cell[3],
                     const int32_t dims[3],
                     float *vertices_out, int32_t *faces_out, int32_t *source, int32_t *cluster,
                     int64_t *counts, void *workspace, void *stream);

/* ---- quadric-error placement of the vertices of a clustered mesh ----
 *
 * rn_mesh_place_quadric: every output vertex of rn_mesh_simplify moves from the mean of its
 * cluster to the point that minimises the weighted sum of its squared distances to the planes of
 * the input faces that touch the cluster, plus a small pull towards the mean (Lindstrom's
 * placement for vertex clustering).  It consumes what rn_mesh_simplify returns -- `cluster` and
 * the mean positions -- and writes new positions for the same output vertices; faces, `source`
 * and the order of everything are rn_mesh_simplify's and stay.
 *
 * cell [3] f64 is a HOST array, the sides of a cell; all other arrays are device memory.
 * vertices_in [nv][3] f32, faces_in [nf][3] i32, cluster [nv] i32 (the output index of each input
 * vertex, anything outside [0, nvo) for none) and positions_in [nvo][3] f32 are never written.
 *   positions_out [nvo][3] f32   the placed vertices; every row is written
 *   counts        [2]      i64   the vertices whose row of positions_out differs in its bits from
 *                                positions_in; the vertices with two or more members that kept
 *                                positions_in's bits because the placement was refused
 * workspace: 8-byte aligned, at least rn_mesh_place_quadric_workspace_bytes(nv, nf, nvo) = 88 nvo
 * bytes (-1 for sizes the entry refuses), laid out [nvo][11] i64: the ten sums S[0..9] and the
 * member count n of every output vertex.  Nothing beyond that size is touched.
 *
 * Every floating-point operation is fp64 and rounded on its own, in the order written (the library
 * is built with -ffp-contract=off); only + - * /, sqrt, rint (to nearest, ties to even),
 * comparisons and conversions occur, so a NumPy restatement gives the same bits
 * (tests/quadric_truth.py).  L = max(cell_x, cell_y, cell_z).
 *
 * 1. Every S and n is 0.
 * 2. Every input vertex v with 0 <= cluster[v] < nvo adds 1 to n of that output vertex.
 * 3. Every input face (i_0, i_1, i_2) with all three indices in [0, nv), a, b, c its corners as
 *    doubles:
 *        e1 = b - a;  e2 = c - a
 *        N_x = e1_y e2_z - e1_z e2_y;  N_y = e1_z e2_x - e1_x e2_z;  N_z = e1_x e2_y - e1_y e2_x
 *        s = (N_x N_x + N_y N_y) + N_z N_z;  len = sqrt(s)
 *    adds nothing unless len is finite and > 0; otherwise
 *        n = N / len;  share = (0.5 len) / (L L);  w = share if share < 1, else 1
 *    and for each corner j = 0, 1, 2 with k = cluster[i_j]: nothing if k is outside [0, nvo) or
 *    equals cluster[i_j'] of an earlier corner j' < j (a face adds once per distinct cluster, and
 *    the faces the clustering drops add too); otherwise, with m = positions_in[k] and p the corner,
 *        r = (p - m) / L   per axis;   nothing unless -2 <= r_i <= 2 on all three axes
 *        d = -((n_x r_x + n_y r_y) + n_z r_z)
 *    (a member and its mean share a cell, so the test on r only refuses a caller's garbage; the
 *    bound below rests on it) and the ten terms
 *        (w n_x) n_x, (w n_x) n_y, (w n_x) n_z, (w n_y) n_y, (w n_y) n_z, (w n_z) n_z,
 *        (w n_x) d, (w n_y) d, (w n_z) d, w
 *    each as the integer rint(term * 2^30), are added to S[0..9] of k by 64-bit integer atomics.
 *    |n_i| <= 1, |r_i| <= 2 and w <= 1 give |d| <= 2 sqrt(3) and |term| < 3.47, so every integer
 *    is below 2^32 in magnitude; one add per face and cluster and nf < 2^30 keep every sum below
 *    2^62.
 * 4. Every output vertex k: positions_in[k]'s BITS if n <= 1 or S[9] == 0.  Otherwise T_i =
 *    (double) S[i] / 2^30 (the conversion to nearest, ties to even), ridge = regularization T_9,
 *        M = [T_0 + ridge, T_1, T_2; T_1, T_3 + ridge, T_4; T_2, T_4, T_5 + ridge],  y = -(T_6, T_7, T_8)
 *    and M x = y by L D L^T without pivoting:
 *        d_0 = M_00;  l_10 = M_01 / d_0;  l_20 = M_02 / d_0
 *        d_1 = M_11 - l_10 M_01;  e = M_12 - l_20 M_01;  l_21 = e / d_1
 *        d_2 = (M_22 - l_20 M_02) - l_21 e
 *        z_0 = y_0;  z_1 = y_1 - l_10 z_0;  z_2 = (y_2 - l_20 z_0) - l_21 z_1
 *        g_i = z_i / d_i
 *        x_2 = g_2;  x_1 = g_1 - l_21 x_2;  x_0 = (g_0 - l_10 x_1) - l_20 x_2
 *    A pivot d_i that is not > 0, or an l or an x that is not finite, gives positions_in's bits.
 *    Then x_i is clamped to +- (max_move cell_i) / L and
 *        out_i = (float) ((double) m_i + L x_i);
 *    an out_i that is not finite gives positions_in's bits for the whole vertex.
 * The ridge makes M positive definite wherever a face added, so no pseudo-inverse and no
 * singular-value threshold are needed: along a direction the planes do not constrain (a flat
 * region, the line of a crease) the vertex stays at the mean.
 *
 * The result is one fixed set of arrays whatever the launch geometry or the order in which the
 * hardware ran the threads.  Whatever faces_in, cluster and the positions hold, nothing is read or
 * written out of bounds, and no loop has a trip count that depends on data.
 *
 * nvo == 0: RN_OK, counts = {0, 0}, no kernel launch.  RN_ERR_INVALID, rn_last_error naming the
 * entry, no launch, outputs untouched: a NULL ctx, nv or nf negative, nv > 2^31 - 2, 3 nf > 2^31 -
 * 1, nvo negative or > nv, a NULL cell, a cell_k not finite or <= 0, regularization outside
 * [2^-20, 1] or NaN, max_move not > 0 (inf is taken), a NULL counts, and with nvo > 0 a NULL
 * vertices_in / cluster / positions_in / positions_out / workspace, a NULL faces_in with nf > 0, a
 * workspace that is not 8-byte aligned, positions_out equal to vertices_in, faces_in, cluster,
 * positions_in or workspace. */
int64_t rn_mesh_place_quadric_workspace_bytes(int64_t nv, int64_t nf, int64_t nvo);
int rn_mesh_place_quadric(rn_ctx *ctx, int64_t nv, const float *vertices_in, int64_t nf,
                          const int32_t *faces_in, const int32_t *cluster, int64_t nvo,
                          const float *positions_in, const double cell[3], double regularization,
                          double max_move, float *positions_out, int64_t *counts, void *workspace,
                          void *stream);

/* ---- the small holes of an indexed triangle mesh capped ----
 *
 * rn_mesh_fill_holes: every simple boundary loop of at most max_edges edges gets a vertex at the
 * mean of its vertices and a fan of faces from that vertex to its edges.
 *
 * All arrays are device memory.  vertices [nv][3] f32, faces [nf][3] i32 and the corner table
 * (offsets [nv + 1] i32, corners [3 nf] i32: the indices c = 3 face + slot of the flattened faces
 * sorted by the vertex they name, and the exclusive prefix of the vertices' corner counts) are
 * never written.  The caller allocates the upper bounds:
 *   new_vertices [nf][3]   f32   the centre of every filled loop
 *   new_faces    [3 nf][3] i32   the faces of the caps, of indices into cat(vertices, new_vertices)
 *   source       [nf]      i32   the label of every filled loop
 *   counts       [5]       i64   filled loops, new faces, loops, loops not simple, boundary
 *                                half-edges
 * Only the first counts[0] rows of new_vertices and source and the first counts[1] rows of
 * new_faces are written; the rest keep their bits.  The caller's mesh after the call is
 * cat(vertices, new_vertices[:counts[0]]) and cat(faces, new_faces[:counts[1]]): the input's order
 * is kept, so per-vertex attributes carry over by position.  workspace: 8-byte aligned, at least
 * rn_mesh_fill_holes_workspace_bytes(nv, nf) bytes (-1 for sizes rn_mesh_fill_holes refuses), laid
 * out scan [nv] u64 | the scan's scratch | total [1] u64 | partial [256][3] i64 | parent, out_deg,
 * in_deg, out_edge, edges, bad [nv] i32 each | status [2] i32 | boundary [3 nf] u8.  Nothing beyond that size is touched.
 *
 * A face COUNTS iff its three indices lie in [0, nv) and differ pairwise.
 *
 * The half-edge h = 3 f + s of a counting face goes from a = faces[f][s] to b = faces[f][(s + 1) %
 * 3].  Over the corners of the counting faces around a, count how often b occurs among the two
 * other vertices of those faces: h is a BOUNDARY half-edge iff that count is exactly 1, that is,
 * iff the undirected edge {a, b} lies in one counting face.  (Duplicate faces have no boundary
 * edges.  The count is the same from either end; the kernel scans the corner list of the end with
 * fewer corners.)
 *
 * The boundary half-edges form a directed graph on the vertices.  A LOOP is a connected component
 * of that graph -- two vertices are connected if a boundary half-edge joins them, in either
 * direction; its LABEL is its smallest vertex, E the number of its boundary half-edges.  A loop is
 * SIMPLE iff every vertex that is an end of one of its half-edges has exactly one outgoing
 * boundary half-edge, exactly one incoming one, and three finite coordinates; such a loop is one
 * directed cycle.  Two holes that meet at a vertex, a rim with a flipped face and a loop through a
 * NaN vertex are not simple and stay open, as a whole.  A loop is FILLED iff it is simple and
 * 3 <= E <= max_edges.  The filled loops are numbered k = 0, 1, ... in ascending label.
 *
 * Filling loop k with label r: walk v_0 = r, v_{j+1} = the head of v_j's outgoing boundary
 * half-edge, for j < E.  The centre is, per axis, the fp64 sum of (double) v_j's f32 coordinate in
 * the walk's order, from 0.0, divided once by (double) E in fp64 and rounded once to f32 (the
 * library is built with -ffp-contract=off; tests/holes_truth.py restates it in NumPy to the bit).
 * new_vertices[k] = the centre, source[k] = r, and the faces (v_{j+1}, v_j, nv + k) for j = 0 ..
 * E - 1, in that order, from row (the sum of E over the filled loops before k) of new_faces: each
 * runs against its boundary half-edge, so the winding is the mesh's.
 *
 * The result is one fixed set of arrays whatever the launch geometry or the order in which the
 * hardware ran the threads (integer atomics only).  Whatever faces, offsets, corners and the
 * positions hold, nothing is read or written out of bounds, no loop waits for another thread, and
 * every chase is bounded (raynet_amd/csrc/raynet_holes_args.h has the proof).  The entry waits for
 * the stream once: RN_ERR_STATE if a chase or a walk met what the definition rules out, which no
 * input can cause.
 *
 * nv == 0 or nf == 0: RN_OK, counts cleared, no kernel launch.  RN_ERR_INVALID, rn_last_error
 * naming the entry, no launch, outputs untouched: nv or nf negative, nv > 2^31 - 2, 3 nf > 2^31 -
 * 1, nv + nf > 2^31 - 2 (a new vertex nv + k is an int32), max_edges < 3 or > 65536, a NULL counts,
 * and with nv > 0 and nf > 0 any other NULL array, a workspace that is not 8-byte aligned, an
 * output (new_vertices, new_faces, source, counts, workspace) that shares a byte with an input or
 * with another output. */
int64_t rn_mesh_fill_holes_workspace_bytes(int64_t nv, int64_t nf);
int rn_mesh_fill_holes(rn_ctx *ctx, int64_t nv, const float *vertices, int64_t nf,
                       const int32_t *faces, const int32_t *offsets, const int32_t *corners,
                       int32_t max_edges,
                       float *new_vertices, int32_t *new_faces, int32_t *source, int64_t *counts,
                       void *workspace, void *stream);

/* ---- an indexed triangle mesh seen from cameras ----
 *
 * rn_mesh_render: for every pixel of V views of H x W pixels the face its ray hits first, the
 * depth of the hit, where in the face it lies, and the vertices' colours and normals there.  All
 * views go in one launch, one lane per pixel.
 *
 * All arrays are device memory; the inputs are never written.
 *   nodes, leaves          the BVH of rn_mesh_build over the triangles vertices[faces[f]] (common.
 *                          mesh_io.get_triangles), so that a leaf's triangle index is a face index
 *   vertices [nv][3] f32, faces [nf][3] i32
 *   colors   [nv][C] f32 or NULL, 1 <= C <= 4;  normals [nv][3] f32 or NULL
 *   cameras  [V][15] f32   per view P_pinv [4][3] | centre [3]: what rn_mesh_depthmap takes
 * Every output is written for all V H W pixels, always:
 *   face   [V][H][W]    i32   the face hit, -1 on a miss
 *   depth  [V][H][W]    f32   0 on a miss
 *   bary   [V][H][W][2] f32   (u, v); (0, 0) on a miss
 *   color  [V][H][W][C] f32   iff colors is given (NULL otherwise); 0 on a miss
 *   normal [V][H][W][3] f32   iff normals is given (NULL otherwise); 0 on a miss
 *
 * The pixel of column x and row y: its ray, its first hit and its depth are rn_mesh_depthmap's --
 * the destination project(P_pinv, (x, y, 1)) formed in float64 from the fp32 P_pinv and rounded
 * once, the first hit of rn_mesh_raycast (the smallest fp32 key, the lower face on equal keys),
 * the float64 distance of the hit to the centre rounded once: depth[view] has the bits
 * rn_mesh_depthmap writes for that view.
 *
 * (u, v) are the fp32 Moeller-Trumbore coordinates of the winning face f, the ones its
 * intersection test computed: with ray the ray's fp32 unit direction, o the centre, p0, p1, p2 the
 * vertices of f, e1 = p1 - p0, e2 = p2 - p0, pvec = ray x e2, inv = 1 / (e1 . pvec), t = o - p0,
 * q = t x e1: u = (t . pvec) inv, v = (ray . q) inv, every dot product ((a + b) + c), every
 * operation fp32 and rounded on its own.  The hit is (1 - u - v) p0 + u p1 + v p2.
 *
 * Interpolation, in fp64, every operation rounded on its own (the library is built with
 * -ffp-contract=off; tests/render_truth.py restates it in NumPy to the bit): U = (double) u,
 * Vb = (double) v, Wb = (1.0 - U) - Vb; per component a = (Wb a0 + U a1) + Vb a2 of the three
 * vertices' values widened to double.  A colour is (float) a.  A normal: l2 = (nx nx + ny ny) +
 * nz nz; (float)(n_k / sqrt(l2)) if l2 > 0 and finite, else (0, 0, 0).
 *
 * A hit face that is not in [0, nf) or names a vertex outside [0, nv) keeps its face and depth and
 * gets bary, color and normal 0.  Whatever faces holds, nothing is read or written out of bounds.
 * The result does not depend on how pixels are dealt to lanes (a wavefront covers an 8 x 8 tile).
 *
 * RN_OK without a launch, nothing written: V == 0, or H W == 0, with valid sizes (whatever the
 * pointers).  RN_ERR_INVALID, rn_last_error naming the entry, no launch, outputs untouched: a
 * negative nv, nf, V, H or W; V > 4096; V H W > 2^31 - 1, or with colors V H W C > 2^31 - 1; C
 * outside 1..4 when colors is given; nv > 2^31 - 2 or 3 nf > 2^31 - 1; nf < 1; with pixels to
 * render a NULL nodes, leaves, vertices, faces, cameras, face, depth or bary, color NULL while
 * colors is not or the reverse, the same for normal and normals. */
int rn_mesh_render(rn_ctx *ctx, const float *nodes, const float *leaves, int64_t nv,
                   const float *vertices, int64_t nf, const int32_t *faces, const float *colors,
                   int32_t C, const float *normals, int32_t V, const float *cameras, int32_t H,
                   int32_t W, int32_t *face, float *depth, float *bary, float *color, float *normal,
                   void *stream);

/* ---- the photographs baked into a texture atlas of a surface mesh ----
 *
 * The atlas (csrc/raynet_texture_args.h, namespace rn_tex; pure integer arithmetic): T is the
 * number of texel steps along a chart's leg, 1 <= T <= 1024.  A cell is S = T + 5 texels square
 * and holds two faces; cells = (nf + 1) / 2, cells_per_row = Cw >= 1 is the caller's, rows =
 * ceil(cells / Cw), Wt = Cw S, Ht = rows S.  Texel centres are at whole coordinates.  The owner of
 * texel (tx, ty): cx = tx / S, i = tx % S, cy = ty / S, j = ty % S, k = cy Cw + cx, lower =
 * (i + j <= T + 3), f = 2 k + (lower ? 0 : 1); a texel with f >= nf is empty.  The corners of a
 * chart in cell-local texels (a, b): lower p0 (1, 1), p1 (T + 1, 1), p2 (1, T + 1); upper
 * p0 (T + 3, T + 3), p1 (3, T + 3), p2 (T + 3, 3).  The point with barycentrics (u, v) for
 * (p1, p2) lies at a = 1 + u T, b = 1 + v T (lower) or a = (T + 3) - u T, b = (T + 3) - v T
 * (upper), so that the 2 x 2 footprint of a bilinear lookup anywhere in a face's chart touches
 * only texels that face owns; the texels a face owns outside its triangle are its gutter.
 *
 * rn_texture_bake: one lane per texel.  All arrays are device memory; the inputs are never
 * written.  vertices [nv][3] f32, faces [nf][3] i32, normals [nv][3] f32 or NULL; cameras, H, W,
 * C, images, depths, tol, min_cos, border and mode are exactly rn_project_colors's.  texture
 * [Ht][Wt][C] f32, weight [Ht][Wt] f32 and views [Ht][Wt] u32 are written for all Ht Wt texels,
 * always, also with V == 0.
 *
 * Per texel with owner f and cell-local (i, j), in fp64, every operation rounded on its own and
 * in the order written (the library is built with -ffp-contract=off; tests/texture_truth.py
 * restates it in NumPy to the bit):
 *   lower:  u0 = (double)(i - 1) / (double)T,        v0 = (double)(j - 1) / (double)T
 *   upper:  u0 = (double)((T + 3) - i) / (double)T,  v0 = (double)((T + 3) - j) / (double)T
 *   u = u0 > 0 ? u0 : 0;  v likewise;  s = u + v;  if s > 1: u = u / s, v = v / s
 *     (a gutter texel takes the colour of a point on its face's rim)
 *   Wb = (1.0 - u) - v;  p_k = (Wb p0_k + u p1_k) + v p2_k of the three vertices widened to
 *     double (rn_mesh_render's interpolation); p is NOT rounded to fp32
 *   the normal: with normals, n_k = (Wb n0_k + u n1_k) + v n2_k; with NULL the face's e1 x e2 of
 *     e1 = p1 - p0, e2 = p2 - p0 in fp64, (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x)
 *     as rn_vertex_area_normals forms it.  It is not normalised (the facing test carries nn); a
 *     zero normal means no facing test and w = 1.
 *   then, for the views in ascending order, rn_project_colors's projection, in-view, facing and
 *     occlusion tests, its bilinear fetch and its blend (mode 0) or best view (mode 1), on that
 *     fp64 point and normal: a NaN fails every test, a view that does not count reads pixel
 *     (0, 0), texture = (float) of the result or 0 where no view counted, weight = (float) den,
 *     views bit v is set iff view v counted.
 * An empty texel gets colour 0, weight 0, views 0, and so does a texel whose face names a vertex
 * outside [0, nv).  Whatever faces holds, nothing is read or written out of bounds.  The result
 * does not depend on how texels are dealt to lanes (a wavefront covers an 8 x 8 tile of texels).
 *
 * RN_OK without a launch, nothing written: nf == 0 with valid scalars (whatever the pointers).
 * RN_ERR_INVALID, rn_last_error naming the entry, no launch, outputs untouched: a negative nv or
 * nf, nv > 2^31 - 2 or 3 nf > 2^31 - 1; T outside 1..1024; cells_per_row outside 1..16384; with
 * faces Wt or Ht > 16384, or Wt Ht C > 2^31 - 1; everything rn_project_colors refuses of V, H, W,
 * C, tol, min_cos, border and mode; with faces a NULL vertices, faces, texture, weight or views,
 * and a NULL cameras or images with V > 0. */
int rn_texture_bake(rn_ctx *ctx, int64_t nv, const float *vertices, int64_t nf, const int32_t *faces,
                    const float *normals, int32_t T, int32_t cells_per_row, int32_t V,
                    const double *cameras, int32_t H, int32_t W, int32_t C, const float *images,
                    const float *depths, double tol, double min_cos, double border, int32_t mode,
                    float *texture, float *weight, uint32_t *views, void *stream);

/* rn_texture_sample: the lookup behind a render, one lane per pixel of rn_mesh_render's face [n]
 * i32 and bary [n][2] f32 planes, flattened; texture [Ht][Wt][C] f32 of the atlas of nf faces, T
 * and cells_per_row; color [n][C] f32 is written for all n pixels.
 *   U = (double) u, Vb = (double) v; lower = (f even), k = f / 2, cx = k % Cw, cy = k / Cw;
 *   a = 1.0 + U (double)T (lower) or (double)(T + 3) - U (double)T (upper), b likewise from Vb;
 *   x = (double)(cx S) + a, y = (double)(cy S) + b
 *   bilinear != 0: x0 = floor(x), x1 = min(x0 + 1, Wt - 1), fx = x - x0, likewise y;
 *     top = t00 + fx (t01 - t00), bot = t10 + fx (t11 - t10), color = (float)(top + fy (bot - top))
 *     of the four texels widened to double
 *   bilinear == 0: the texel at (rint(x), rint(y)), half to even.
 * Colour 0 for a face outside [0, nf) (-1 is one) and for U or Vb outside [0, 1] (a NaN is).
 * Every load lies inside the atlas whatever the inputs hold.
 *
 * RN_OK without a launch, nothing written: n == 0 with valid scalars.  RN_ERR_INVALID,
 * rn_last_error naming the entry, no launch, color untouched: a negative n or nf, 3 nf > 2^31 - 1;
 * T or cells_per_row out of range; C outside 1..4; bilinear neither 0 nor 1; n C > 2^31 - 1; with
 * faces Wt or Ht > 16384 or Wt Ht C > 2^31 - 1; with pixels a NULL face, bary or color, and a NULL
 * texture with nf > 0. */
int rn_texture_sample(rn_ctx *ctx, int64_t n, const int32_t *face, const float *bary, int64_t nf,
                      int32_t T, int32_t cells_per_row, int32_t C, const float *texture,
                      int32_t bilinear, float *color, void *stream);

/* hipEvent pair on `stream`; rn_timer_stop returns elapsed milliseconds after
 * synchronising on the stop event (bench.py's per-kernel timing). */
int rn_timer_start(rn_ctx *ctx, void *stream);
int rn_timer_stop(rn_ctx *ctx, void *stream, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* RAYNET_HIP_H */
