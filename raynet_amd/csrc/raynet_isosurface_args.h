// raynet_isosurface_args.h -- the size arithmetic and the argument checks of rn_isosurface_count /
// rn_isosurface_emit (raynet_isosurface.inl), host-only and free of HIP so that they compile into a
// stand-alone program (tests/isosurface_args_main.cpp, built with the address and
// undefined-behaviour sanitizers by tests/test_isosurface_cpu.py, which also checks the scan's
// arithmetic, raynet_scan_args.h's).  The launchers act on the verdicts and lay the workspace out
// with these functions; the kernels guard their output rows with row_in().
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_scan_args.h"

namespace rn_iso {

using rn_scan::scan_levels, rn_scan::scan_scratch_words;

enum Verdict { INVALID = -1, EMPTY = 0, LAUNCH = 1 };

// The lattice of a [gx][gy][gz] grid: its points, closed: one more on either side of every axis.
struct Lattice {
    int64_t nx, ny, nz;
    int64_t points;     // L = nx ny nz
    int64_t cells;      // (nx - 1)(ny - 1)(nz - 1): 0 where an axis has a single point
};

constexpr Lattice lattice(int32_t gx, int32_t gy, int32_t gz, int32_t closed) {
    const int64_t c = closed ? 2 : 0;
    const int64_t nx = (int64_t)gx + c, ny = (int64_t)gy + c, nz = (int64_t)gz + c;
    return Lattice{nx, ny, nz, nx * ny * nz, (nx - 1) * (ny - 1) * (nz - 1)};
}

// A point carries at most 7 vertices and a cell at most 12 triangles: with 12 L < 2^31 every
// index of the outputs is an int32 and the two running counts share one 64-bit word without a
// carry between its halves.
constexpr bool lattice_fits(const Lattice &l) {
    return l.nx >= 1 && l.ny >= 1 && l.nz >= 1 &&
           l.points <= (((int64_t)1 << 31) - 1) / 12;      // (no product that could overflow)
}
constexpr int64_t max_vertices(const Lattice &l) { return l.cells > 0 ? 7 * l.points : 0; }
constexpr int64_t max_faces(const Lattice &l) { return 12 * l.cells; }

// ---- the workspace: 64-bit words first, the bytes of the edge masks behind them ----
//   counts  [L]        u64   (vertices << 32 | triangles) per point, then their exclusive scan
//   scratch [scan_scratch_words(L)] u64
//   total   [1]        u64
//   masks   [L]        u8    bit d - 1: the edge (p, d) carries a vertex
constexpr size_t ws_counts(const Lattice &) { return 0; }
constexpr size_t ws_scratch(const Lattice &l) { return 8 * (size_t)l.points; }
constexpr size_t ws_total(const Lattice &l) {
    return ws_scratch(l) + 8 * (size_t)scan_scratch_words(l.points);
}
constexpr size_t ws_masks(const Lattice &l) { return ws_total(l) + 8; }
constexpr int64_t workspace_bytes(const Lattice &l) {
    return lattice_fits(l) ? (int64_t)((ws_masks(l) + (size_t)l.points + 7) / 8 * 8) : -1;
}

// what both entries ask of the inputs
inline bool inputs_ok(bool have_ctx, const Lattice &l, const void *belief, float iso,
                      int32_t closed, const void *workspace) {
    if (!have_ctx || !belief || !workspace) return false;
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return false;      // 64-bit words
    if (closed != 0 && closed != 1) return false;
    if (!std::isfinite(iso)) return false;
    if (closed && !(iso > 0.0f)) return false;      // the padding's 0 must be outside
    return lattice_fits(l);
}

// rn_isosurface_count: EMPTY (both totals 0, no launch) for a lattice without cells
inline Verdict count_args(bool have_ctx, const Lattice &l, const void *belief, float iso,
                          int32_t closed, const void *workspace, const void *totals_host) {
    if (!inputs_ok(have_ctx, l, belief, iso, closed, workspace) || !totals_host) return INVALID;
    return l.cells > 0 ? LAUNCH : EMPTY;
}

// rn_isosurface_emit: nv / nf are a count's totals, so within what the lattice can give
inline Verdict emit_args(bool have_ctx, const Lattice &l, const void *belief, float iso,
                         int32_t closed, const void *workspace, int64_t nv, int64_t nf,
                         const void *vertices_out, const void *faces_out) {
    if (!inputs_ok(have_ctx, l, belief, iso, closed, workspace)) return INVALID;
    if (nv < 0 || nf < 0 || nv > max_vertices(l) || nf > max_faces(l)) return INVALID;
    if (nv == 0 && nf == 0) return EMPTY;
    if ((nv > 0 && !vertices_out) || (nf > 0 && !faces_out)) return INVALID;
    return LAUNCH;
}

// (constexpr: the kernel guards and addresses its rows with the same functions)
// row `row` of an output of n rows may be written
constexpr bool row_in(int64_t row, int64_t n) { return row >= 0 && row < n; }
constexpr size_t row_index(int64_t row, int column) { return 3 * (size_t)row + (size_t)column; }
// floats of `vertices` / int32s of `faces` the kernel may touch
constexpr size_t rows_extent(int64_t n) { return n > 0 ? row_index(n - 1, 2) + 1 : 0; }

// the two halves of a count word
constexpr uint64_t pack_counts(uint32_t vertices, uint32_t faces) {
    return ((uint64_t)vertices << 32) | faces;
}
constexpr int64_t count_vertices(uint64_t w) { return (int64_t)(w >> 32); }
constexpr int64_t count_faces(uint64_t w) { return (int64_t)(w & 0xffffffffu); }

}  // namespace rn_iso
