// raynet_quadric_args.h -- the argument checks, the workspace layout and the four phases of
// rn_mesh_place_quadric (raynet_quadric.inl): the sums cleared, the members of every output vertex
// counted, the plane of every face added to the quadric of each cluster it touches, and the 3 x 3
// system of every output vertex solved.  Host-only and free of HIP so that they compile into a
// stand-alone program (tests/quadric_args_main.cpp, built with the address and
// undefined-behaviour sanitizers by tests/test_quadric_cpu.py).  The launcher acts on the verdict
// and lays the workspace out with these functions; the kernels call clear / count_member /
// add_face / solve_vertex and add the index of the thread and the atomics policy.  The functions
// are constexpr only so that the device may call them; nothing here is evaluated at compile time.
// The limits of the sizes, the guards of the indices and the launch geometry are
// raynet_mesh_args.h's.
//
// The definition is in include/raynet_hip.h at rn_mesh_place_quadric.
// Every floating-point operation below is fp64, written as one operation per rounding and in the
// definition's order; the library is built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_mesh_args.h"

namespace rn_qd {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::sizes_ok, rn_mesh::blocks;
using rn_mesh::vertex_in, rn_mesh::face_in, rn_mesh::xyz_index;

constexpr int WORDS = 11;               // S [10] i64 | n i64 per output vertex
constexpr int COUNT = 10;               // the word of n
constexpr int64_t VERTEX_BYTES = 8 * WORDS;
constexpr double FIXED_ONE = 1073741824.0;          // 2^30: the fixed-point unit of a term
// 1.5 * 2^52: for |x| < 2^51 the sum x + 1.5 * 2^52 lies in [2^52, 2^53), where the doubles are
// the whole numbers, so the sum and the difference are rint(x), ties to even, of either sign
constexpr double ROUND_SHIFT = 6755399441055744.0;
constexpr double MIN_REGULARIZATION = 9.5367431640625e-07;      // 2^-20
constexpr double REACH = 2.0;           // a corner farther than this many L from its cluster's
                                        // position, along any axis, adds nothing
constexpr double LARGEST = 1.7976931348623157e308;

// finite: neither a NaN (which fails both comparisons) nor an infinity, host and device alike
constexpr bool is_finite(double x) { return x >= -LARGEST && x <= LARGEST; }

// ---- the workspace: sums [nvo][11] i64 ----
constexpr int64_t workspace_bytes(int64_t nv, int64_t nf, int64_t nvo) {
    if (!sizes_ok(nv, nf) || nvo < 0 || nvo > nv) return -1;
    return (VERTEX_BYTES * nvo + 7) / 8 * 8;
}
constexpr size_t word_index(int64_t k, int word) { return (size_t)WORDS * (size_t)k + (size_t)word; }

// rn_mesh_place_quadric.  The scalars and the host array first, then nvo == 0 (only `counts` is
// written: EMPTY, whatever the other pointers), then the pointers.
inline Verdict place_args(bool have_ctx, int64_t nv, const void *vertices_in, int64_t nf,
                          const void *faces_in, const void *cluster, int64_t nvo,
                          const void *positions_in, const double *cell, double regularization,
                          double max_move, const void *positions_out, const void *counts,
                          const void *workspace) {
    if (!have_ctx || !sizes_ok(nv, nf) || nvo < 0 || nvo > nv) return INVALID;
    if (!cell) return INVALID;
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(cell[k]) || !(cell[k] > 0.0)) return INVALID;
    if (!(regularization >= MIN_REGULARIZATION) || !(regularization <= 1.0)) return INVALID;
    if (!(max_move > 0.0)) return INVALID;
    if (!counts) return INVALID;
    if (nvo == 0) return EMPTY;
    if (!vertices_in || !cluster || !positions_in || !positions_out || !workspace) return INVALID;
    if (nf > 0 && !faces_in) return INVALID;
    if ((uintptr_t)workspace % 8 != 0) return INVALID;
    if (positions_out == positions_in || positions_out == vertices_in ||
        positions_out == cluster || positions_out == workspace) return INVALID;
    if (nf > 0 && positions_out == faces_in) return INVALID;
    return LAUNCH;
}

// what the solve needs, by value
struct Solve {
    double cell[3];
    double L;               // max(cell)
    double regularization, max_move;
};
inline Solve solve_of(const double *cell, double regularization, double max_move) {
    double L = cell[0];
    if (cell[1] > L) L = cell[1];
    if (cell[2] > L) L = cell[2];
    return Solve{{cell[0], cell[1], cell[2]}, L, regularization, max_move};
}

// what the kernels share, by value
struct Tables {
    int64_t nv, nf, nvo;
    int64_t *sums;          // [nvo][11]
};
inline Tables tables_of(int64_t nv, int64_t nf, int64_t nvo, void *workspace) {
    return Tables{nv, nf, nvo, (int64_t *)workspace};
}

// ---- phase 1, one thread per output vertex ----
constexpr void clear(int64_t k, const Tables &t) {
    for (int i = 0; i < WORDS; i++) t.sums[word_index(k, i)] = 0;
}

// ---- phase 2, one thread per input vertex: one integer atomic at its output vertex.
// A: add_i64(p, x) ----
template <class A>
constexpr void count_member(const A &at, int64_t v, const int32_t *cluster, const Tables &t) {
    const int64_t k = cluster[v];
    if (vertex_in(k, t.nvo)) at.add_i64(t.sums + word_index(k, COUNT), 1);
}

// a term in fixed point: rint(term * 2^30), ties to even, for |term| < 2^21
constexpr int64_t fixed(double term) {
    const double scaled = term * FIXED_ONE;
    const double shifted = scaled + ROUND_SHIFT;
    return (int64_t)(shifted - ROUND_SHIFT);
}
// (a term of 0 changes no sum: the atomic is left out)
template <class A>
constexpr void add_term(const A &at, const Tables &t, int64_t k, int word, double term) {
    const int64_t q = fixed(term);
    if (q != 0) at.add_i64(t.sums + word_index(k, word), q);
}

// ---- phase 3, one thread per input face: its weighted plane into the ten sums of every distinct
// cluster among its corners.  |n| <= 1, |r_i| <= 2 and w <= 1 give |d| <= 2 sqrt(3) and every
// |term| < 3.47, so |q| < 2^32; one add per face and cluster and nf < 2^30 keep |S| < 2^62 ----
template <class A>
constexpr void add_face(const A &at, int64_t f, const float *vertices, const int32_t *faces,
                        const int32_t *cluster, const float *positions, double L,
                        const Tables &t) {
    const int64_t i0 = faces[xyz_index(f, 0)];
    if (!vertex_in(i0, t.nv)) return;
    const int64_t i1 = faces[xyz_index(f, 1)];
    if (!vertex_in(i1, t.nv)) return;
    const int64_t i2 = faces[xyz_index(f, 2)];
    if (!vertex_in(i2, t.nv)) return;
    const int64_t corner[3] = {i0, i1, i2};
    double p[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) p[j][i] = (double)vertices[xyz_index(corner[j], i)];
    const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const double ax = e1y * e2z, bx = e1z * e2y, Nx = ax - bx;
    const double ay = e1z * e2x, by = e1x * e2z, Ny = ay - by;
    const double az = e1x * e2y, bz = e1y * e2x, Nz = az - bz;
    const double sx = Nx * Nx, sy = Ny * Ny, sz = Nz * Nz;
    const double sxy = sx + sy, s = sxy + sz;
    const double len = std::sqrt(s);
    if (!is_finite(len) || !(len > 0.0)) return;
    const double nx = Nx / len, ny = Ny / len, nz = Nz / len;
    const double half = 0.5 * len, LL = L * L, share = half / LL;
    const double w = share < 1.0 ? share : 1.0;         // (a NaN share -- 0 / 0 -- weighs 1)
    const double wx = w * nx, wy = w * ny, wz = w * nz;
    int64_t seen[3] = {-1, -1, -1};
    for (int j = 0; j < 3; j++) {
        const int64_t k = cluster[corner[j]];
        seen[j] = k;
        if (!vertex_in(k, t.nvo)) continue;
        if ((j > 0 && k == seen[0]) || (j > 1 && k == seen[1])) continue;
        const double rx = (p[j][0] - (double)positions[xyz_index(k, 0)]) / L;
        const double ry = (p[j][1] - (double)positions[xyz_index(k, 1)]) / L;
        const double rz = (p[j][2] - (double)positions[xyz_index(k, 2)]) / L;
        // (a NaN fails the test: a corner or a position that is not finite adds nothing)
        if (!(rx >= -REACH && rx <= REACH && ry >= -REACH && ry <= REACH && rz >= -REACH &&
              rz <= REACH))
            continue;
        const double dx = nx * rx, dy = ny * ry, dz = nz * rz;
        const double dxy = dx + dy, dot = dxy + dz;
        const double d = -dot;
        add_term(at, t, k, 0, wx * nx);
        add_term(at, t, k, 1, wx * ny);
        add_term(at, t, k, 2, wx * nz);
        add_term(at, t, k, 3, wy * ny);
        add_term(at, t, k, 4, wy * nz);
        add_term(at, t, k, 5, wz * nz);
        add_term(at, t, k, 6, wx * d);
        add_term(at, t, k, 7, wy * d);
        add_term(at, t, k, 8, wz * d);
        add_term(at, t, k, 9, w);
    }
}

// M x = y for the symmetric M = L D L^T, without pivoting: false for a pivot that is not > 0 (a
// NaN is not) or a factor or a solution that is not finite
constexpr bool solve_ldlt(double m00, double m01, double m02, double m11, double m12, double m22,
                          double y0, double y1, double y2, double *x) {
    const double d0 = m00;
    if (!(d0 > 0.0)) return false;
    const double l10 = m01 / d0, l20 = m02 / d0;
    const double u11 = l10 * m01, d1 = m11 - u11;
    if (!(d1 > 0.0)) return false;
    const double u12 = l20 * m01, e = m12 - u12;
    const double l21 = e / d1;
    const double u22 = l20 * m02, v22 = m22 - u22, w22 = l21 * e, d2 = v22 - w22;
    if (!(d2 > 0.0)) return false;
    if (!is_finite(l10) || !is_finite(l20) || !is_finite(l21)) return false;
    // L z = y
    const double z0 = y0;
    const double a1 = l10 * z0, z1 = y1 - a1;
    const double a2 = l20 * z0, b2 = y2 - a2, c2 = l21 * z1, z2 = b2 - c2;
    // D g = z
    const double g0 = z0 / d0, g1 = z1 / d1, g2 = z2 / d2;
    // L^T x = g
    const double x2 = g2;
    const double h1 = l21 * x2, x1 = g1 - h1;
    const double h0 = l10 * x1, i0 = g0 - h0, j0 = l20 * x2, x0 = i0 - j0;
    if (!is_finite(x0) || !is_finite(x1) || !is_finite(x2)) return false;
    x[0] = x0;
    x[1] = x1;
    x[2] = x2;
    return true;
}

constexpr double clamped(double x, double limit) {
    return x > limit ? limit : (x < -limit ? -limit : x);
}

// whether two floats have the same bits (-0 and +0 do not)
constexpr bool same_bits(float a, float b) {
    return __builtin_bit_cast(uint32_t, a) == __builtin_bit_cast(uint32_t, b);
}

// ---- phase 4, one thread per output vertex: plain loads of its eleven words, its row of
// positions_out, and the two tallies by integer atomics.  A: count(p), which adds 1 ----
template <class A>
constexpr void solve_vertex(const A &at, int64_t k, const float *positions_in, const Solve &s,
                            const Tables &t, float *positions_out, int64_t *counts) {
    const int64_t n = t.sums[word_index(k, COUNT)];
    bool placed = false;
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (n > 1 && t.sums[word_index(k, 9)] != 0) {
        double T[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < 10; i++) T[i] = (double)t.sums[word_index(k, i)] / FIXED_ONE;
        const double ridge = s.regularization * T[9];
        double x[3] = {0.0, 0.0, 0.0};
        placed = solve_ldlt(T[0] + ridge, T[1], T[2], T[3] + ridge, T[4], T[5] + ridge, -T[6],
                            -T[7], -T[8], x);
        for (int i = 0; i < 3 && placed; i++) {
            const double reach = s.max_move * s.cell[i];
            const double limit = reach / s.L;
            const double step = s.L * clamped(x[i], limit);
            const double at_i = (double)positions_in[xyz_index(k, i)] + step;
            out[i] = (float)at_i;
            placed = is_finite((double)out[i]);
        }
    }
    if (!placed) {
        // the bits of positions_in (a copy of a float changes none, as in rn_sp::emit_vertex)
        for (int i = 0; i < 3; i++)
            positions_out[xyz_index(k, i)] = positions_in[xyz_index(k, i)];
        if (n > 1) at.count(counts + 1);
        return;
    }
    bool moved = false;
    for (int i = 0; i < 3; i++) {
        positions_out[xyz_index(k, i)] = out[i];
        moved = moved || !same_bits(out[i], positions_in[xyz_index(k, i)]);
    }
    if (moved) at.count(counts);
}

}  // namespace rn_qd
