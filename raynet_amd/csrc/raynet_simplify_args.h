// raynet_simplify_args.h -- the argument checks, the workspace layout, the cell of a vertex, the
// sums of a cell, the mean, the face predicate and the emission of rn_mesh_simplify
// (raynet_simplify.inl), host-only and free of HIP so that they compile into a stand-alone program
// (tests/simplify_args_main.cpp, built with the address and undefined-behaviour sanitizers by
// tests/test_simplify_cpu.py).  The launcher acts on the verdict and lays the workspace out with
// these functions; the kernels call clear_cell / place_vertex and add_to_cell / flag_face /
// emit_vertex / emit_face and add the index of the thread, the atomics policy and, in the binning,
// the sums over the lanes of a wavefront that share a cell (the host program bins vertex by vertex
// with bin_vertex: integer sums, the same words).  The functions are constexpr only so that the
// device may call them; nothing here is evaluated at compile time.  The limits of the sizes, the
// guards of the indices and the launch geometry are raynet_mesh_args.h's, the size of the scan's
// scratch raynet_scan_args.h's.
//
// The definition is in include/raynet_hip.h at rn_mesh_simplify.  Every
// floating-point operation below is fp64, written as one operation per rounding and in the
// definition's order; the library is built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_mesh_args.h"
#include "raynet_scan_args.h"

namespace rn_sp {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::MAX_BLOCKS, rn_mesh::sizes_ok, rn_mesh::blocks;
using rn_mesh::vertex_in, rn_mesh::face_in, rn_mesh::xyz_index;

constexpr double FIXED_ONE = 2097152.0; // 2^21: the fixed-point unit of a position inside its cell
constexpr double ROUND_SHIFT = 4503599627370496.0;    // 2^52: x + 2^52 - 2^52 rounds x to a whole number
constexpr int32_t NO_REP = 2147483647;  // the `rep` of a cell nobody was binned into
constexpr int64_t CELL_BYTES = 32;      // S [3] u64 | rep i32 | n i32

// ---- the grid: with the sizes, what rn_mesh_simplify_workspace_bytes refuses ----
// the number of cells, or -1 for a dims the entry refuses (no product that could overflow)
constexpr int64_t cell_count(const int32_t *dims) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return -1;
    const int64_t xy = (int64_t)dims[0] * dims[1];
    if (xy > INT32_LIMIT) return -1;
    const int64_t all = xy * dims[2];
    return all > INT32_LIMIT ? -1 : all;
}

// ---- the workspace, 64-bit words first:
//   table   [cells][4] u64   S_x, S_y, S_z, then rep (low i32) | n (high i32): 32 bytes per cell
//   fscan   [nf]       u64   the kept flag of every face, then its exclusive scan
//   vscan   [nv]       u64   1 at the smallest vertex of every used cluster, then its scan
//   scratch [rn_scan::scan_scratch_words(max(nv, nf))] u64   (the two scans run one after the other)
//   cell_of [nv]       i32   the cell of every binned vertex, -1 for a singleton
constexpr int64_t ws_table(int64_t, int64_t, int64_t) { return 0; }
constexpr int64_t ws_fscan(int64_t, int64_t, int64_t cells) { return CELL_BYTES * cells; }
constexpr int64_t ws_vscan(int64_t nv, int64_t nf, int64_t cells) {
    return ws_fscan(nv, nf, cells) + 8 * nf;
}
constexpr int64_t ws_scratch(int64_t nv, int64_t nf, int64_t cells) {
    return ws_vscan(nv, nf, cells) + 8 * nv;
}
constexpr int64_t ws_cell_of(int64_t nv, int64_t nf, int64_t cells) {
    return ws_scratch(nv, nf, cells) + 8 * rn_scan::scan_scratch_words(nv > nf ? nv : nf);
}
constexpr int64_t workspace_bytes(int64_t nv, int64_t nf, const int32_t *dims) {
    const int64_t cells = cell_count(dims);
    if (!sizes_ok(nv, nf) || cells < 0) return -1;
    return (ws_cell_of(nv, nf, cells) + 4 * nv + 7) / 8 * 8;
}

// rn_mesh_simplify.  The scalars and the three host arrays first, then nv == 0 (only `counts` is
// written: EMPTY, whatever the other pointers), then the pointers; `source` and `cluster` may be
// null and are not looked at here.
inline Verdict simplify_args(bool have_ctx, int64_t nv, const void *vertices_in, int64_t nf,
                             const void *faces_in, const double *origin, const double *cell,
                             const int32_t *dims, const void *vertices_out, const void *faces_out,
                             const void *counts, const void *workspace) {
    if (!have_ctx || !sizes_ok(nv, nf)) return INVALID;
    if (!origin || !cell || cell_count(dims) < 0) return INVALID;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(cell[k]) || !(cell[k] > 0.0)) return INVALID;
        if (!std::isfinite(origin[k])) return INVALID;
    }
    if (!counts) return INVALID;
    if (nv == 0) return EMPTY;
    if (!vertices_in || !vertices_out || !workspace) return INVALID;
    if (nf > 0 && (!faces_in || !faces_out)) return INVALID;
    if ((uintptr_t)workspace % 8 != 0) return INVALID;
    if (vertices_out == vertices_in || (nf > 0 && faces_out == faces_in)) return INVALID;
    if (vertices_out == workspace || (nf > 0 && faces_out == workspace)) return INVALID;
    return LAUNCH;
}

// ---- what the kernels guard and address the table with (the mesh: rn_mesh's guards) ----
constexpr bool cell_in(int64_t c, int64_t cells) { return c >= 0 && c < cells; }
constexpr size_t sum_index(int64_t cell, int axis) { return 4 * (size_t)cell + (size_t)axis; }
constexpr size_t rep_index(int64_t cell) { return 8 * (size_t)cell + 6; }   // as an i32 array
constexpr size_t n_index(int64_t cell) { return 8 * (size_t)cell + 7; }

// the grid as the kernels carry it, by value
struct Grid {
    double origin[3], cell[3];
    int32_t dims[3];
    int64_t cells;
};
inline Grid grid_of(const double *origin, const double *cell, const int32_t *dims) {
    return Grid{{origin[0], origin[1], origin[2]}, {cell[0], cell[1], cell[2]},
                {dims[0], dims[1], dims[2]}, cell_count(dims)};
}

// what the kernels share, by value
struct Tables {
    int64_t nv, nf;
    uint64_t *table;        // [cells][4]
    int32_t *table32;       // the same words as i32: rep and n
    uint64_t *fscan, *vscan;
    int32_t *cell_of;
};
inline Tables tables_of(int64_t nv, int64_t nf, int64_t cells, void *workspace) {
    char *w = (char *)workspace;
    return Tables{nv, nf, (uint64_t *)(w + ws_table(nv, nf, cells)),
                  (int32_t *)(w + ws_table(nv, nf, cells)),
                  (uint64_t *)(w + ws_fscan(nv, nf, cells)),
                  (uint64_t *)(w + ws_vscan(nv, nf, cells)),
                  (int32_t *)(w + ws_cell_of(nv, nf, cells))};
}

// ---- the cell of a position: q and w per axis; false for a singleton (a NaN fails every test) ----
struct Place {
    int64_t cell;           // -1 for a singleton
    uint64_t w[3];
};
constexpr bool axis_place(double p, double origin, double cell, int32_t dim, int64_t *q,
                          uint64_t *w) {
    const double t = (p - origin) / cell;
    // 0 <= floor(t) < dim iff 0 <= t < dim, dim being a whole number; a NaN and either infinity
    // fail here.  For such a t the truncating conversion is floor(t), and for 0 <= x <= 2^21 the
    // sum and difference with 2^52 is rint(x), ties to even: two roundings, both as the definition
    // has them, in a form that host and device compile alike.
    if (!(t >= 0.0) || !(t < (double)dim)) return false;
    *q = (int64_t)t;
    const double u = t - (double)*q;
    const double scaled = u * FIXED_ONE;
    const double shifted = scaled + ROUND_SHIFT;
    *w = (uint64_t)(shifted - ROUND_SHIFT);
    return true;
}
constexpr Place place_of(const float *vertices, int64_t v, const Grid &g) {
    Place p{-1, {0, 0, 0}};
    int64_t q[3] = {0, 0, 0};
    bool in = true;
    for (int k = 0; k < 3; k++)
        in = axis_place((double)vertices[xyz_index(v, k)], g.origin[k], g.cell[k], g.dims[k],
                        &q[k], &p.w[k]) && in;
    if (in) p.cell = (q[0] * g.dims[1] + q[1]) * g.dims[2] + q[2];
    return p;
}

// ---- phase 1, one thread per cell ----
constexpr void clear_cell(int64_t c, const Tables &t) {
    t.table[sum_index(c, 0)] = 0;
    t.table[sum_index(c, 1)] = 0;
    t.table[sum_index(c, 2)] = 0;
    t.table32[rep_index(c)] = NO_REP;
    t.table32[n_index(c)] = 0;
}

// ---- phase 2, one thread per vertex: its cell into cell_of, its flag cleared, and for a binned
// vertex the five integer atomics at its cell.  A: min_i32(p, x), add_i32(p, x), add_u64(p, x) ----
// the place of vertex v, stored: its cell (or -1) into cell_of, its flag cleared
constexpr Place place_vertex(int64_t v, const float *vertices, const Grid &g, const Tables &t) {
    Place p = place_of(vertices, v, g);
    if (!cell_in(p.cell, g.cells)) p.cell = -1;
    t.cell_of[v] = (int32_t)p.cell;
    t.vscan[v] = 0;
    return p;
}
// n binned vertices of one cell, the smallest of them `rep`, their w summed in S: the five atomics
template <class A>
constexpr void add_to_cell(const A &at, const Tables &t, int64_t cell, int32_t rep, int32_t n,
                           uint64_t Sx, uint64_t Sy, uint64_t Sz) {
    at.min_i32(t.table32 + rep_index(cell), rep);
    at.add_i32(t.table32 + n_index(cell), n);
    at.add_u64(t.table + sum_index(cell, 0), Sx);
    at.add_u64(t.table + sum_index(cell, 1), Sy);
    at.add_u64(t.table + sum_index(cell, 2), Sz);
}
// one vertex on its own (the host program's phase; the kernel adds the vertices of a wavefront
// that share a cell together: integer sums, the same words in any grouping)
template <class A>
constexpr void bin_vertex(const A &at, int64_t v, const float *vertices, const Grid &g,
                          const Tables &t) {
    const Place p = place_vertex(v, vertices, g, t);
    if (p.cell >= 0) add_to_cell(at, t, p.cell, (int32_t)v, 1, p.w[0], p.w[1], p.w[2]);
}

// the cluster of vertex v of [0, nv), named by its smallest member: the rep of its cell, v itself
// for a singleton.  (cell_of and rep are this call's own; they are checked all the same, so that
// no address depends on them unchecked.)
constexpr int64_t cluster_of(int64_t v, const Tables &t, int64_t cells) {
    const int64_t c = t.cell_of[v];
    if (!cell_in(c, cells)) return v;
    const int64_t r = t.table32[rep_index(c)];
    return vertex_in(r, t.nv) ? r : v;
}

// the face predicate: the three clusters of a kept face in k[], false for a dropped one
constexpr bool face_clusters(int64_t f, const int32_t *faces, const Tables &t, int64_t cells,
                             int64_t *k) {
    const int64_t i0 = faces[xyz_index(f, 0)], i1 = faces[xyz_index(f, 1)],
                  i2 = faces[xyz_index(f, 2)];
    if (!vertex_in(i0, t.nv) || !vertex_in(i1, t.nv) || !vertex_in(i2, t.nv)) return false;
    k[0] = cluster_of(i0, t, cells);
    k[1] = cluster_of(i1, t, cells);
    k[2] = cluster_of(i2, t, cells);
    return k[0] != k[1] && k[1] != k[2] && k[0] != k[2];
}

// ---- phase 3, one thread per face: the kept flag, and 1 at the three clusters of a kept face
// (plain stores: every writer stores the same value) ----
constexpr void flag_face(int64_t f, const int32_t *faces, const Tables &t, int64_t cells) {
    int64_t k[3] = {0, 0, 0};
    const bool kept = face_clusters(f, faces, t, cells, k);
    t.fscan[f] = kept ? 1 : 0;
    if (!kept) return;
    t.vscan[k[0]] = 1;
    t.vscan[k[1]] = 1;
    t.vscan[k[2]] = 1;
}

// (phase 4: the exclusive scans of fscan and vscan, their totals into counts[1] and counts[0])

// whether the scanned flag of vertex v was 1: the step to the next entry, the total behind the last
constexpr bool was_flagged(const uint64_t *scan, int64_t i, int64_t n, uint64_t total) {
    return (i + 1 < n ? scan[i + 1] : total) != scan[i];
}

// the mean of a cell along one axis
constexpr float cell_mean(double origin, double cell, int64_t q, uint64_t S, int32_t n) {
    const double m = (double)S / (double)n;
    const double in_cell = m / FIXED_ONE;
    const double at = (double)q + in_cell;
    const double x = origin + cell * at;
    return (float)x;
}

// ---- phase 5, one thread per vertex: cluster[v], and for the smallest vertex of a used cluster
// its row of vertices_out and source ----
constexpr void emit_vertex(int64_t v, const float *vertices, const Grid &g, const Tables &t,
                           const int64_t *counts, float *vertices_out, int32_t *source,
                           int32_t *cluster) {
    const uint64_t total = (uint64_t)counts[0];
    const int64_t k = cluster_of(v, t, g.cells);
    const bool used = was_flagged(t.vscan, k, t.nv, total);
    const int64_t out = (int64_t)t.vscan[k];
    if (cluster) cluster[v] = used && vertex_in(out, t.nv) ? (int32_t)out : -1;
    if (!used || k != v || !vertex_in(out, t.nv)) return;
    if (source) source[out] = (int32_t)v;
    const int64_t c = t.cell_of[v];
    const int32_t n = cell_in(c, g.cells) ? t.table32[n_index(c)] : 1;
    if (n <= 1) {
        vertices_out[xyz_index(out, 0)] = vertices[xyz_index(v, 0)];
        vertices_out[xyz_index(out, 1)] = vertices[xyz_index(v, 1)];
        vertices_out[xyz_index(out, 2)] = vertices[xyz_index(v, 2)];
        return;
    }
    const int64_t qz = c % g.dims[2], qy = c / g.dims[2] % g.dims[1],
                  qx = c / g.dims[2] / g.dims[1];
    vertices_out[xyz_index(out, 0)] =
        cell_mean(g.origin[0], g.cell[0], qx, t.table[sum_index(c, 0)], n);
    vertices_out[xyz_index(out, 1)] =
        cell_mean(g.origin[1], g.cell[1], qy, t.table[sum_index(c, 1)], n);
    vertices_out[xyz_index(out, 2)] =
        cell_mean(g.origin[2], g.cell[2], qz, t.table[sum_index(c, 2)], n);
}

// ---- phase 6, one thread per face: a kept face's row of faces_out ----
constexpr void emit_face(int64_t f, const int32_t *faces, const Tables &t, int64_t cells,
                         int32_t *faces_out) {
    int64_t k[3] = {0, 0, 0};
    if (!face_clusters(f, faces, t, cells, k)) return;
    const int64_t out = (int64_t)t.fscan[f];
    if (!face_in(out, t.nf)) return;
    faces_out[xyz_index(out, 0)] = (int32_t)t.vscan[k[0]];
    faces_out[xyz_index(out, 1)] = (int32_t)t.vscan[k[1]];
    faces_out[xyz_index(out, 2)] = (int32_t)t.vscan[k[2]];
}

}  // namespace rn_sp
