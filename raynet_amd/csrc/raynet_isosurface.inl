// raynet_isosurface.inl -- the surface of a belief grid: an indexed triangle mesh by marching
// tetrahedra over the Kuhn split of every lattice cell (the definition is in
// include/raynet_hip.h at rn_isosurface_count).  Included at the end of raynet_hip.hip.
//
//   k_iso_classify  one thread per lattice point: the eight values of its cell (0 outside the
//                   grid), the 7-bit mask of its edges (p, d) that carry a vertex and the
//                   triangles of its cell, as one count word (vertices << 32 | triangles).
//   scan_exclusive_u64
//                   the library's grid-level exclusive scan of the count words (raynet_scan.inl).
//   k_iso_emit      one thread per lattice point: its vertices at its vertex offset, its cell's
//                   triangles at its triangle offset; the vertex of an edge is found at
//                   offset[q] + popcount(mask[q] & ((1 << (d - 1)) - 1)).
//
// Plain HIP C++.  Every fp32 operation of the definition is rounded on its own and in the stated
// order (-ffp-contract=off; the divisions are IEEE): tests/isosurface_truth.py restates it in
// np.float32 and the GPU tests ask for the same bits, in the same order.

#include "raynet_isosurface_args.h"

namespace {

// The triangles of a tetrahedron: [tetrahedron][inside pattern of its four corners], derived and
// checked by tools/isosurface_table.py.  Bits 0-1: how many; 3 bits per entry, triangle 0 from
// bit 2, triangle 1 from bit 11: the edge (l, m) of local corners as its index in
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  (Read per lane from constant memory: a vector load.)
__constant__ uint32_t ISO_TRI[96] = {
    0x00000, 0x00221, 0x00381, 0x70c46, 0x00565, 0xac2a2, 0x34582, 0x00589,
     0x004a9, 0x94522, 0xa83a2, 0x003a5, 0x50c66, 0x00461, 0x00141, 0x00000,
    0x00000, 0x00141, 0x00461, 0x8ca86, 0x003a5, 0x74542, 0xa44a2, 0x004a9,
     0x00589, 0xb01a2, 0x54562, 0x00565, 0x88b86, 0x00381, 0x00221, 0x00000,
    0x00000, 0x00141, 0x00461, 0x8ca86, 0x003a5, 0x74542, 0xa44a2, 0x004a9,
     0x00589, 0xb01a2, 0x54562, 0x00565, 0x88b86, 0x00381, 0x00221, 0x00000,
    0x00000, 0x00221, 0x00381, 0x70c46, 0x00565, 0xac2a2, 0x34582, 0x00589,
     0x004a9, 0x94522, 0xa83a2, 0x003a5, 0x50c66, 0x00461, 0x00141, 0x00000,
    0x00000, 0x00221, 0x00381, 0x70c46, 0x00565, 0xac2a2, 0x34582, 0x00589,
     0x004a9, 0x94522, 0xa83a2, 0x003a5, 0x50c66, 0x00461, 0x00141, 0x00000,
    0x00000, 0x00141, 0x00461, 0x8ca86, 0x003a5, 0x74542, 0xa44a2, 0x004a9,
     0x00589, 0xb01a2, 0x54562, 0x00565, 0x88b86, 0x00381, 0x00221, 0x00000,
};

// the Kuhn split: corner masks of the six tetrahedra (bit 0: +x, bit 1: +y, bit 2: +z)
constexpr int ISO_TET[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7},
                               {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
constexpr int ISO_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};

struct IsoGeom {
    int gx, gy, gz;     // the grid
    int c;              // closed: the lattice starts one point in front of the grid
    int nx, ny, nz;     // the lattice
    int L;              // its points (12 L < 2^31)
};

// The cell of a lattice point: the values at p + d (v[0] its own), which of those points the
// lattice has, and which are inside.
struct IsoCell {
    float v[8];
    unsigned exists, inside;
    int i, j, k;

    __device__ __forceinline__ void load(const IsoGeom &g, const float *__restrict__ belief,
                                         float iso, int p) {
        k = p % g.nz;
        const int ij = p / g.nz;
        j = ij % g.ny;
        i = ij / g.ny;
        exists = 0;
        inside = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int li = i + (d & 1), lj = j + ((d >> 1) & 1), lk = k + ((d >> 2) & 1);
            const int x = li - g.c, y = lj - g.c, z = lk - g.c;
            const bool in_grid = (unsigned)x < (unsigned)g.gx && (unsigned)y < (unsigned)g.gy &&
                                 (unsigned)z < (unsigned)g.gz;
            // (the load is always of the grid: entry 0 stands in where the point is outside)
            const int64_t at = in_grid ? ((int64_t)x * g.gy + y) * g.gz + z : 0;
            const float b = belief[at];
            v[d] = in_grid ? b : 0.0f;
            exists |= (unsigned)(li < g.nx && lj < g.ny && lk < g.nz) << d;
            inside |= (unsigned)(v[d] >= iso) << d;              // NaN: outside
        }
    }
    // bit d - 1: the edge (p, d) carries a vertex
    __device__ __forceinline__ unsigned edge_mask() const {
        const unsigned differs = (inside & 1u) ? ~inside : inside;
        return ((differs & exists) >> 1) & 0x7fu;
    }
    __device__ __forceinline__ bool is_base() const { return exists == 0xffu; }
    __device__ __forceinline__ unsigned triangles() const {
        unsigned n = 0;
        if (is_base()) {
#pragma unroll
            for (int t = 0; t < 6; t++) {
                constexpr unsigned one = 1u;
                const unsigned corners = (one << ISO_TET[t][0]) | (one << ISO_TET[t][1]) |
                                         (one << ISO_TET[t][2]) | (one << ISO_TET[t][3]);
                const unsigned in = (unsigned)__popc(inside & corners);
                n += min(in, 4u - in);
            }
        }
        return n;
    }
};

__global__ __launch_bounds__(BLOCK) void k_iso_classify(IsoGeom g, const float *__restrict__ belief,
                                                        float iso, uint64_t *counts,
                                                        uint8_t *masks) {
    const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (p >= g.L) return;
    IsoCell cell;
    cell.load(g, belief, iso, (int)p);
    const unsigned mask = cell.edge_mask();
    counts[p] = rn_iso::pack_counts((uint32_t)__popc(mask), cell.triangles());
    masks[p] = (uint8_t)mask;
}

// --------------------------------------------------------------------------- the mesh
// coordinate of lattice point `at` of one axis: the table inside the grid, one voxel size in
// front of its first / behind its last entry for the padded points (the read is always of the
// table)
__device__ __forceinline__ float iso_coordinate(const float *__restrict__ table, int g, int c,
                                                float h, int at) {
    const int v = at - c;
    const float a = table[min(max(v, 0), g - 1)];
    return v < 0 ? a - h : (v >= g ? a + h : a);
}

// entry `which` of e.  (As a sum of masked terms, which is the same integer: a chain of selects
// between the members the compiler turns back into an indexed table, kept in LDS.)
__device__ __forceinline__ int iso_pick(const int (&e)[6], unsigned which) {
    return (which == 0 ? e[0] : 0) + (which == 1 ? e[1] : 0) + (which == 2 ? e[2] : 0) +
           (which == 3 ? e[3] : 0) + (which == 4 ? e[4] : 0) + (which == 5 ? e[5] : 0);
}

__global__ __launch_bounds__(BLOCK) void k_iso_emit(IsoGeom g, const float *__restrict__ belief,
                                                    float iso, const float *__restrict__ axes,
                                                    float hx, float hy, float hz,
                                                    const uint64_t *__restrict__ offsets,
                                                    const uint8_t *__restrict__ masks, int64_t nv,
                                                    int64_t nf, float *vertices, int32_t *faces) {
    const int64_t p = blockIdx.x * (int64_t)BLOCK + threadIdx.x;
    if (p >= g.L) return;
    IsoCell cell;
    cell.load(g, belief, iso, (int)p);
    const uint64_t own = offsets[p];
    const unsigned mask = cell.edge_mask();
    if (mask) {
        const float x0 = iso_coordinate(axes, g.gx, g.c, hx, cell.i),
                    x1 = iso_coordinate(axes, g.gx, g.c, hx, cell.i + 1),
                    y0 = iso_coordinate(axes + g.gx, g.gy, g.c, hy, cell.j),
                    y1 = iso_coordinate(axes + g.gx, g.gy, g.c, hy, cell.j + 1),
                    z0 = iso_coordinate(axes + g.gx + g.gy, g.gz, g.c, hz, cell.k),
                    z1 = iso_coordinate(axes + g.gx + g.gy, g.gz, g.c, hz, cell.k + 1);
        const float a = cell.v[0];
        int64_t row = rn_iso::count_vertices(own);
#pragma unroll
        for (int d = 1; d < 8; d++) {
            if ((mask >> (d - 1)) & 1u) {
                const float t = (iso - a) / (cell.v[d] - a);
                if (rn_iso::row_in(row, nv)) {
                    vertices[rn_iso::row_index(row, 0)] = (d & 1) ? x0 + t * (x1 - x0) : x0;
                    vertices[rn_iso::row_index(row, 1)] = (d & 2) ? y0 + t * (y1 - y0) : y0;
                    vertices[rn_iso::row_index(row, 2)] = (d & 4) ? z0 + t * (z1 - z0) : z0;
                }
                row++;
            }
        }
    }
    if (!cell.is_base() || cell.inside == 0u || cell.inside == 0xffu) return;
    // the seven points edges of this cell start from: their vertex offsets and edge masks
    int first[7];
    unsigned edges[7];
#pragma unroll
    for (int lo = 0; lo < 7; lo++) {
        const int64_t q = p + (int64_t)(lo & 1) * g.ny * g.nz + ((lo >> 1) & 1) * g.nz +
                          ((lo >> 2) & 1);
        first[lo] = (int)rn_iso::count_vertices(offsets[q]);
        edges[lo] = masks[q];
    }
    int64_t row = rn_iso::count_faces(own);
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const unsigned pattern = ((cell.inside >> ISO_TET[t][0]) & 1u) |
                                 (((cell.inside >> ISO_TET[t][1]) & 1u) << 1) |
                                 (((cell.inside >> ISO_TET[t][2]) & 1u) << 2) |
                                 (((cell.inside >> ISO_TET[t][3]) & 1u) << 3);
        if (pattern == 0u || pattern == 15u) continue;
        const uint32_t word = ISO_TRI[16 * t + pattern];
        int e[6];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int lo = ISO_TET[t][ISO_EDGE[k][0]], d = ISO_TET[t][ISO_EDGE[k][1]] ^ lo;
            e[k] = first[lo] + __popc(edges[lo] & ((1u << (d - 1)) - 1u));
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if ((unsigned)r < (word & 3u)) {
                if (rn_iso::row_in(row, nf)) {
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        faces[rn_iso::row_index(row, k)] =
                            iso_pick(e, (word >> (2 + 9 * r + 3 * k)) & 7u);
                }
                row++;
            }
        }
    }
}

IsoGeom iso_geom(const rn_ctx *ctx, const rn_iso::Lattice &l, int32_t closed) {
    IsoGeom g;
    g.gx = ctx->p.gx; g.gy = ctx->p.gy; g.gz = ctx->p.gz;
    g.c = closed;
    g.nx = (int)l.nx; g.ny = (int)l.ny; g.nz = (int)l.nz;
    g.L = (int)l.points;
    return g;
}

}  // namespace

extern "C" {

int64_t rn_isosurface_workspace_bytes(rn_ctx *ctx, int32_t closed) {
    if (!ctx || (closed != 0 && closed != 1)) return -1;
    return rn_iso::workspace_bytes(rn_iso::lattice(ctx->p.gx, ctx->p.gy, ctx->p.gz, closed));
}

int rn_isosurface_count(rn_ctx *ctx, const float *belief, float iso, int32_t closed,
                        void *workspace, int64_t *totals_host, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    const rn_iso::Lattice l = rn_iso::lattice(ctx->p.gx, ctx->p.gy, ctx->p.gz, closed);
    const rn_iso::Verdict v =
        rn_iso::count_args(true, l, belief, iso, closed, workspace, totals_host);
    if (v == rn_iso::INVALID)
        return fail(ctx, RN_ERR_INVALID, "rn_isosurface_count: bad argument (iso %g, closed %d, "
                    "lattice %lld points)", (double)iso, (int)closed, (long long)l.points);
    totals_host[0] = totals_host[1] = 0;
    if (v == rn_iso::EMPTY) return RN_OK;
    int rc = need_axes(ctx);
    if (rc) return rc;
    char *ws = static_cast<char *>(workspace);
    uint64_t *counts = reinterpret_cast<uint64_t *>(ws + rn_iso::ws_counts(l));
    uint64_t *scratch = reinterpret_cast<uint64_t *>(ws + rn_iso::ws_scratch(l));
    uint64_t *total = reinterpret_cast<uint64_t *>(ws + rn_iso::ws_total(l));
    uint8_t *masks = reinterpret_cast<uint8_t *>(ws + rn_iso::ws_masks(l));
    const dim3 grid((unsigned)rn_scan::scan_tiles(l.points));
    hipLaunchKernelGGL(k_iso_classify, grid, dim3(BLOCK), 0, S(stream), iso_geom(ctx, l, closed),
                       belief, iso, counts, masks);
    RN_LAUNCH_CHECK(ctx);
    rc = scan_exclusive_u64(ctx, counts, l.points, scratch, total, S(stream));
    if (rc) return rc;
    uint64_t sum = 0;
    RN_HIP(ctx, hipMemcpyAsync(&sum, total, sizeof(sum), hipMemcpyDeviceToHost, S(stream)));
    RN_HIP(ctx, hipStreamSynchronize(S(stream)));
    totals_host[0] = rn_iso::count_vertices(sum);
    totals_host[1] = rn_iso::count_faces(sum);
    return RN_OK;
}

int rn_isosurface_emit(rn_ctx *ctx, const float *belief, float iso, int32_t closed,
                       const void *workspace, int64_t nv, int64_t nf, float *vertices_out,
                       int32_t *faces_out, void *stream) {
    if (!ctx) return RN_ERR_INVALID;
    const rn_iso::Lattice l = rn_iso::lattice(ctx->p.gx, ctx->p.gy, ctx->p.gz, closed);
    const rn_iso::Verdict v = rn_iso::emit_args(true, l, belief, iso, closed, workspace, nv, nf,
                                                vertices_out, faces_out);
    if (v == rn_iso::EMPTY) return RN_OK;
    if (v != rn_iso::LAUNCH)
        return fail(ctx, RN_ERR_INVALID, "rn_isosurface_emit: bad argument (iso %g, closed %d, "
                    "nv %lld, nf %lld)", (double)iso, (int)closed, (long long)nv, (long long)nf);
    int rc = need_axes(ctx);
    if (rc) return rc;
    const char *ws = static_cast<const char *>(workspace);
    const uint64_t *offsets = reinterpret_cast<const uint64_t *>(ws + rn_iso::ws_counts(l));
    const uint8_t *masks = reinterpret_cast<const uint8_t *>(ws + rn_iso::ws_masks(l));
    const Params &p = ctx->p;
    // the voxel sizes of the padded points: fl(fl(max - min) / g), on the host as in the header
    const float hx = (p.bbox[3] - p.bbox[0]) / (float)p.gx,
                hy = (p.bbox[4] - p.bbox[1]) / (float)p.gy,
                hz = (p.bbox[5] - p.bbox[2]) / (float)p.gz;
    const dim3 grid((unsigned)rn_scan::scan_tiles(l.points));
    hipLaunchKernelGGL(k_iso_emit, grid, dim3(BLOCK), 0, S(stream), iso_geom(ctx, l, closed),
                       belief, iso, (const float *)ctx->axes, hx, hy, hz, offsets, masks, nv, nf,
                       vertices_out, faces_out);
    RN_LAUNCH_CHECK(ctx);
    return RN_OK;
}

}  // extern "C"
