// raynet_holes_args.h -- the argument checks, the workspace layout, the boundary test of a
// half-edge, the tally of a loop, the scan word of a filled loop and the walk that caps it, of
// rn_mesh_fill_holes (raynet_holes.inl), host-only and free of HIP so that they compile into a
// stand-alone program (tests/holes_args_main.cpp, built with the address and undefined-behaviour
// sanitizers by tests/test_holes_cpu.py).  The launcher acts on the verdict and lays the workspace
// out with these functions; the kernels call init_vertex / mark_edge / tally_edge / flag_vertex /
// emit_loop (tally_of where the lanes of a wavefront add together) and add the index of the thread
// and the atomics policies.  The functions are constexpr
// only so that the device may call them; nothing here is evaluated at compile time.  The limits of
// the sizes, the guards of the indices and the launch geometry are raynet_mesh_args.h's, the
// union-find raynet_components_args.h's, the size of the scan's scratch raynet_scan_args.h's.
//
// The definition is in include/raynet_hip.h at rn_mesh_fill_holes.  The
// centre of a loop is the one floating-point result: an fp64 sum in the walk's order, one fp64
// division, one rounding to fp32; the library is built with -ffp-contract=off.
//
// Two atomics policies, both template parameters.  U is the union-find's (load / cas / store on
// `parent`, raynet_components_args.h).  A has
//     void A::add_i32(int32_t *p, int32_t x) const      *p += x
//     void A::min_i32(int32_t *p, int32_t x) const      *p = min(*p, x)
//     void A::add_i64(int64_t *p, int64_t x) const      *p += x
// integer read-modify-writes whose results nobody reads in the launch that issues them: every word
// they touch has one fixed value when the launch ends, whatever the order of the threads.
//
// No loop waits, every chase is bounded:
//   * The unions are section 22's: parent[x] <= x at all times, every write lowers a word, every
//     chase follows strictly decreasing indices and ends within nv steps; a failed compare-and-swap
//     is another thread's progress.  Flattening runs in a launch of its own, after which
//     parent[v] is the smallest vertex of v's component of the boundary graph and is not written
//     again.
//   * The scan of a corner list takes offsets[v + 1] - offsets[v] steps, both ends cut to
//     [0, 3 nf]: at most 3 nf, whatever `offsets` holds.
//   * The walk of a loop takes exactly E <= max_edges steps: E is a number read once, not a
//     condition on what the walk meets.  It follows out_edge, which mark_edge wrote from `faces`
//     alone: out_edge[v] is the smallest boundary half-edge that leaves v, so it leaves v.  In a
//     loop that is filled every vertex has one boundary half-edge out and one in and the loop is
//     connected: one directed cycle of E half-edges, on which E steps from r end at r.  A walk that
//     meets anything else -- a word that names no boundary half-edge of its vertex, an end other
//     than r -- stops, sets the status word and leaves an error to the launcher; no input can cause
//     that, it is the belt of section 22 again.
//   * Nothing spins on a word another thread writes: tally, flags and walk read only what an
//     earlier launch finished.
// Every index that addresses something is checked where it is used, also the workspace's own words
// (parent, out_edge, the scan word): vertex_in, corner_in, clamp_slot, and the ranges of the
// outputs in emit_loop.
#pragma once

#include <cstddef>
#include <cstdint>

#include "raynet_components_args.h"
#include "raynet_mesh_args.h"
#include "raynet_scan_args.h"

namespace rn_hl {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::MAX_BLOCKS, rn_mesh::sizes_ok, rn_mesh::blocks;
using rn_mesh::vertex_in, rn_mesh::face_in, rn_mesh::corner_in, rn_mesh::clamp_slot;
using rn_mesh::xyz_index;

constexpr int32_t MIN_EDGES = 3;            // the smallest loop there is
constexpr int32_t MAX_EDGES = 65536;        // the longest loop a call may ask to fill
constexpr int32_t NO_EDGE = 2147483647;     // the out_edge of a vertex no boundary half-edge leaves
constexpr int COUNTS = 5;   // filled loops, new faces, loops, loops not simple, boundary half-edges
constexpr int SLOTS = 256;  // partial sums of counts[2..4]: one per workgroup modulo SLOTS

// ---- the sizes: sizes_ok, and every new vertex nv + k (k < nf: a filled loop has three
// half-edges or more, and there are at most 3 nf) is an int32 like the others ----
constexpr bool fill_sizes_ok(int64_t nv, int64_t nf) {
    return sizes_ok(nv, nf) && nv + nf <= INT32_LIMIT - 1;
}

// ---- the workspace, 64-bit words first:
//   scan     [nv] u64   the scan word of every vertex, then its exclusive scan
//   scratch  [rn_scan::scan_scratch_words(nv)] u64
//   total    [1]  u64   the sum of the scan words: filled loops << 32 | new faces
//   partial  [SLOTS][3] i64   the labels' parts of counts[2..4], spread over SLOTS places so that
//                       the atomics of thousands of labels do not meet on three words
//   parent, out_deg, in_deg, out_edge, edges, bad   [nv] i32 each
//   status   [2]  i32   [0]: 1 when a chase or a walk met what the definition rules out
//   boundary [3 nf] u8  1 for a boundary half-edge
constexpr int64_t ws_scan(int64_t, int64_t) { return 0; }
constexpr int64_t ws_scratch(int64_t nv, int64_t) { return 8 * nv; }
constexpr int64_t ws_total(int64_t nv, int64_t nf) {
    return ws_scratch(nv, nf) + 8 * rn_scan::scan_scratch_words(nv);
}
constexpr int64_t ws_partial(int64_t nv, int64_t nf) { return ws_total(nv, nf) + 8; }
constexpr int64_t partial_bytes() { return 8 * 3 * SLOTS; }
constexpr int64_t ws_parent(int64_t nv, int64_t nf) { return ws_partial(nv, nf) + partial_bytes(); }
constexpr int64_t ws_out_deg(int64_t nv, int64_t nf) { return ws_parent(nv, nf) + 4 * nv; }
constexpr int64_t ws_in_deg(int64_t nv, int64_t nf) { return ws_parent(nv, nf) + 8 * nv; }
constexpr int64_t ws_out_edge(int64_t nv, int64_t nf) { return ws_parent(nv, nf) + 12 * nv; }
constexpr int64_t ws_edges(int64_t nv, int64_t nf) { return ws_parent(nv, nf) + 16 * nv; }
constexpr int64_t ws_bad(int64_t nv, int64_t nf) { return ws_parent(nv, nf) + 20 * nv; }
constexpr int64_t ws_status(int64_t nv, int64_t nf) { return ws_parent(nv, nf) + 24 * nv; }
constexpr int64_t ws_boundary(int64_t nv, int64_t nf) { return ws_status(nv, nf) + 8; }
constexpr int64_t workspace_bytes(int64_t nv, int64_t nf) {
    if (!fill_sizes_ok(nv, nf)) return -1;
    return (ws_boundary(nv, nf) + 3 * nf + 7) / 8 * 8;
}

// whether the byte ranges [p, p + pn) and [q, q + qn) share a byte (an empty range shares none)
inline bool overlap(const void *p, int64_t pn, const void *q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn > 0 && qn > 0 && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

// rn_mesh_fill_holes.  The scalars first, then `counts`, then nv == 0 and nf == 0 (only `counts` is
// written: EMPTY, whatever the other pointers), then the pointers and that no output shares a byte
// with an input or with another output.
inline Verdict fill_args(bool have_ctx, int64_t nv, const void *vertices, int64_t nf,
                         const void *faces, const void *offsets, const void *corners,
                         int32_t max_edges, const void *new_vertices, const void *new_faces,
                         const void *source, const void *counts, const void *workspace) {
    if (!have_ctx || !fill_sizes_ok(nv, nf)) return INVALID;
    if (max_edges < MIN_EDGES || max_edges > MAX_EDGES) return INVALID;
    if (!counts) return INVALID;
    if (nv == 0 || nf == 0) return EMPTY;
    if (!vertices || !faces || !offsets || !corners) return INVALID;
    if (!new_vertices || !new_faces || !source || !workspace) return INVALID;
    if ((uintptr_t)workspace % 8 != 0) return INVALID;
    const void *in[4] = {vertices, faces, offsets, corners};
    const int64_t in_bytes[4] = {12 * nv, 12 * nf, 4 * (nv + 1), 12 * nf};
    const void *out[5] = {new_vertices, new_faces, source, counts, workspace};
    const int64_t out_bytes[5] = {12 * nf, 36 * nf, 4 * nf, 8 * COUNTS, workspace_bytes(nv, nf)};
    for (int i = 0; i < 5; i++) {
        for (int j = 0; j < 4; j++)
            if (overlap(out[i], out_bytes[i], in[j], in_bytes[j])) return INVALID;
        for (int j = i + 1; j < 5; j++)
            if (overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return INVALID;
    }
    return LAUNCH;
}

// what the kernels share, by value
struct Tables {
    int64_t nv, nf;
    int32_t max_edges;
    uint64_t *scan, *total;
    int64_t *partial;
    int32_t *parent, *out_deg, *in_deg, *out_edge, *edges, *bad, *status;
    uint8_t *boundary;
};
inline Tables tables_of(int64_t nv, int64_t nf, int32_t max_edges, void *workspace) {
    char *w = (char *)workspace;
    return Tables{nv, nf, max_edges,
                  (uint64_t *)(w + ws_scan(nv, nf)), (uint64_t *)(w + ws_total(nv, nf)),
                  (int64_t *)(w + ws_partial(nv, nf)),
                  (int32_t *)(w + ws_parent(nv, nf)), (int32_t *)(w + ws_out_deg(nv, nf)),
                  (int32_t *)(w + ws_in_deg(nv, nf)), (int32_t *)(w + ws_out_edge(nv, nf)),
                  (int32_t *)(w + ws_edges(nv, nf)), (int32_t *)(w + ws_bad(nv, nf)),
                  (int32_t *)(w + ws_status(nv, nf)), (uint8_t *)(w + ws_boundary(nv, nf))};
}

// ---- which faces count: three indices in [0, nv), pairwise different ----
constexpr bool face_counts(int64_t nv, int64_t a, int64_t b, int64_t c) {
    return vertex_in(a, nv) && vertex_in(b, nv) && vertex_in(c, nv) && a != b && b != c && a != c;
}
// x - x is 0 for a finite x and NaN for a NaN and for either infinity
constexpr bool finite(float x) { return x - x == 0.0f; }
constexpr bool finite3(const float *vertices, int64_t v) {
    return finite(vertices[xyz_index(v, 0)]) && finite(vertices[xyz_index(v, 1)]) &&
           finite(vertices[xyz_index(v, 2)]);
}

// ---- phase 1, one thread per vertex ----
constexpr void init_vertex(int64_t v, const Tables &t) {
    t.parent[v] = (int32_t)v;
    t.out_deg[v] = 0;
    t.in_deg[v] = 0;
    t.out_edge[v] = NO_EDGE;
    t.edges[v] = 0;
    t.bad[v] = 0;
    if (v == 0) {
        t.status[0] = 0;
        t.total[0] = 0;
    }
}

// ---- the boundary test ----
// the corners `offsets` gives vertex v, cut to the entries `corners` has (below 0: none)
constexpr int64_t corner_count(int64_t v, int64_t nf, const int32_t *offsets) {
    return clamp_slot(offsets[v + 1], nf) - clamp_slot(offsets[v], nf);
}
// how often q occurs among the two other vertices of the counting faces around p
constexpr int32_t faces_sharing(int64_t p, int64_t q, int64_t nv, int64_t nf, const int32_t *faces,
                                const int32_t *offsets, const int32_t *corners) {
    int32_t n = 0;
    const int64_t first = clamp_slot(offsets[p], nf), last = clamp_slot(offsets[p + 1], nf);
    for (int64_t k = first; k < last; k++) {
        const int64_t c = corners[k];
        if (!corner_in(c, nf)) continue;
        const int64_t g = c / 3;
        const int slot = (int)(c % 3);
        const int64_t i0 = faces[xyz_index(g, 0)], i1 = faces[xyz_index(g, 1)],
                      i2 = faces[xyz_index(g, 2)];
        if (!face_counts(nv, i0, i1, i2)) continue;
        if (faces[xyz_index(g, slot)] != p) continue;       // (a table that is not this mesh's)
        if (faces[xyz_index(g, (slot + 1) % 3)] == q) n++;
        if (faces[xyz_index(g, (slot + 2) % 3)] == q) n++;
    }
    return n;
}
// the half-edge h = 3 f + s of [0, 3 nf): false for one of a face that does not count, else its
// ends in *a -> *b
constexpr bool half_edge(int64_t h, int64_t nv, const int32_t *faces, int64_t *a, int64_t *b) {
    const int64_t f = h / 3;
    const int s = (int)(h % 3);
    const int64_t i0 = faces[xyz_index(f, 0)], i1 = faces[xyz_index(f, 1)],
                  i2 = faces[xyz_index(f, 2)];
    if (!face_counts(nv, i0, i1, i2)) return false;
    *a = faces[xyz_index(f, s)];
    *b = faces[xyz_index(f, (s + 1) % 3)];
    return true;
}
// a -> b is a boundary half-edge iff {a, b} lies in exactly one counting face; the corner list of
// the end with fewer corners is scanned (the first end on a tie)
constexpr bool is_boundary(int64_t a, int64_t b, int64_t nv, int64_t nf, const int32_t *faces,
                           const int32_t *offsets, const int32_t *corners) {
    const bool from_a = corner_count(a, nf, offsets) <= corner_count(b, nf, offsets);
    return faces_sharing(from_a ? a : b, from_a ? b : a, nv, nf, faces, offsets, corners) == 1;
}

// ---- phase 2, one thread per half-edge: its flag; a boundary half-edge a -> b also counts at
// both ends, offers itself as a's way out and joins a and b.  false when the union-find reached
// its bound ----
template <class A, class U>
constexpr bool mark_edge(const A &at, const U &uf, int64_t h, const int32_t *faces,
                         const int32_t *offsets, const int32_t *corners, const Tables &t) {
    int64_t a = 0, b = 0;
    const bool on = half_edge(h, t.nv, faces, &a, &b) &&
                    is_boundary(a, b, t.nv, t.nf, faces, offsets, corners);
    t.boundary[h] = on ? 1 : 0;
    if (!on) return true;
    at.add_i32(t.out_deg + a, 1);
    at.add_i32(t.in_deg + b, 1);
    at.min_i32(t.out_edge + a, (int32_t)h);
    return rn_cc::unite(uf, (int32_t)a, (int32_t)b, rn_cc::step_bound(t.nv));
}

// (phase 3: rn_cc::flatten per vertex, in a launch of its own)

// ---- phase 4, one thread per half-edge: a boundary half-edge counts at its loop's label, and
// marks the loop if one of its ends has more or less than one boundary half-edge out and one in,
// or a coordinate that is not finite ----
constexpr bool plain_vertex(int64_t v, const float *vertices, const Tables &t) {
    return t.out_deg[v] == 1 && t.in_deg[v] == 1 && finite3(vertices, v);
}
// what half-edge h adds: its loop's label, -1 for a half-edge that is not on the boundary, and whether
// one of its ends is not plain
struct Tally {
    int64_t label;
    bool bad;
};
constexpr Tally tally_of(int64_t h, const float *vertices, const int32_t *faces, const Tables &t) {
    if (!t.boundary[h]) return Tally{-1, false};
    int64_t a = 0, b = 0;
    if (!half_edge(h, t.nv, faces, &a, &b)) return Tally{-1, false};
    const int64_t r = t.parent[a];
    if (!vertex_in(r, t.nv)) return Tally{-1, false};
    return Tally{r, !plain_vertex(a, vertices, t) || !plain_vertex(b, vertices, t)};
}
// one half-edge on its own (the host program's phase; the kernel adds the half-edges of a wavefront
// that share a label together: integer sums, the same words in any grouping).  `bad` counts the
// half-edges with an end that is not plain; only whether it is 0 is read.
template <class A>
constexpr void tally_edge(const A &at, int64_t h, const float *vertices, const int32_t *faces,
                          const Tables &t) {
    const Tally y = tally_of(h, vertices, faces, t);
    if (y.label < 0) return;
    at.add_i32(t.edges + y.label, 1);
    if (y.bad) at.add_i32(t.bad + y.label, 1);
}

// ---- the scan word: loops in the high half, faces in the low half (their sum is at most
// 3 nf < 2^31: the low half never carries) ----
constexpr uint64_t scan_word(int32_t E) { return ((uint64_t)1 << 32) | (uint64_t)(uint32_t)E; }
constexpr int64_t word_loops(uint64_t w) { return (int64_t)(w >> 32); }
constexpr int64_t word_faces(uint64_t w) { return (int64_t)(w & 0xffffffffu); }
// vertex v is the label of a loop
constexpr bool is_label(int64_t v, const Tables &t) { return t.parent[v] == v && t.edges[v] > 0; }
// ... of one that is filled
constexpr bool is_filled(int64_t v, const Tables &t) {
    return is_label(v, t) && t.bad[v] == 0 && t.edges[v] >= MIN_EDGES && t.edges[v] <= t.max_edges;
}

// ---- phase 5, one thread per vertex: its scan word, and a label's part of counts[2..4] into the
// partial sums of `slot` in [0, SLOTS) (the launcher cleared them; any slot gives the same totals) ----
template <class A>
constexpr void flag_vertex(const A &at, int64_t v, const Tables &t, int slot) {
    t.scan[v] = is_filled(v, t) ? scan_word(t.edges[v]) : 0;
    if (!is_label(v, t) || slot < 0 || slot >= SLOTS) return;
    int64_t *part = t.partial + 3 * slot;
    at.add_i64(part + 0, 1);
    if (t.bad[v] != 0) at.add_i64(part + 1, 1);
    at.add_i64(part + 2, t.edges[v]);
}

// (phase 6: the exclusive scan of `scan`, its total into `total`)

// ---- phase 7, one thread per vertex: vertex 0 takes the total apart into counts[0..1] and adds the
// partial sums up into counts[2..4]; the label
// of a filled loop walks it, E steps: its faces, its centre, its source.  false when the walk met
// what the definition rules out (nothing more is written then) ----
constexpr bool emit_loop(int64_t v, const float *vertices, const int32_t *faces, const Tables &t,
                         int64_t *counts, float *new_vertices, int32_t *new_faces,
                         int32_t *source) {
    if (v == 0) {
        counts[0] = word_loops(t.total[0]);
        counts[1] = word_faces(t.total[0]);
        int64_t sums[3] = {0, 0, 0};
        for (int i = 0; i < 3 * SLOTS; i++) sums[i % 3] += t.partial[i];
        counts[2] = sums[0];
        counts[3] = sums[1];
        counts[4] = sums[2];
    }
    if (!is_filled(v, t)) return true;
    const int64_t E = t.edges[v], k = word_loops(t.scan[v]), base = word_faces(t.scan[v]);
    if (!face_in(k, t.nf) || base + E > 3 * t.nf || t.nv + k > INT32_LIMIT - 1) return false;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t at = v;
    for (int64_t j = 0; j < E; j++) {
        const int64_t h = t.out_edge[at];
        if (!corner_in(h, t.nf) || !t.boundary[h]) return false;
        int64_t a = 0, b = 0;
        if (!half_edge(h, t.nv, faces, &a, &b) || a != at) return false;
        sx = sx + (double)vertices[xyz_index(at, 0)];
        sy = sy + (double)vertices[xyz_index(at, 1)];
        sz = sz + (double)vertices[xyz_index(at, 2)];
        new_faces[xyz_index(base + j, 0)] = (int32_t)b;
        new_faces[xyz_index(base + j, 1)] = (int32_t)at;
        new_faces[xyz_index(base + j, 2)] = (int32_t)(t.nv + k);
        at = b;
    }
    if (at != v) return false;
    const double n = (double)E;
    new_vertices[xyz_index(k, 0)] = (float)(sx / n);
    new_vertices[xyz_index(k, 1)] = (float)(sy / n);
    new_vertices[xyz_index(k, 2)] = (float)(sz / n);
    source[k] = (int32_t)v;
    return true;
}

}  // namespace rn_hl
