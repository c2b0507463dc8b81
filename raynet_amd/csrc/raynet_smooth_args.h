// raynet_smooth_args.h -- the argument checks, the workspace layout, the ping-pong parity, the ring
// entry of a table position and the step of one vertex of rn_mesh_smooth (raynet_smooth.inl),
// host-only and free of HIP so that they compile into a stand-alone program
// (tests/smooth_args_main.cpp, built with the address and undefined-behaviour sanitizers by
// tests/test_smooth_cpu.py).  The launcher acts on the verdict and walks the steps with
// step_factor / step_source / step_target; the kernels call ring_entry and step_vertex and add
// nothing of their own beyond the index of the thread.  The limits of the sizes, the guards of the
// indices and the launch geometry are raynet_mesh_args.h's.  The functions are constexpr only so that
// the device may call them; nothing here is evaluated at compile time.
//
// The definition is in include/raynet_hip.h at rn_mesh_smooth.  Every
// floating-point operation below is fp64, written as one operation per rounding and in the
// definition's order; the library is built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "raynet_mesh_args.h"

namespace rn_sm {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::MAX_BLOCKS, rn_mesh::sizes_ok, rn_mesh::blocks;
using rn_mesh::vertex_in, rn_mesh::corner_in, rn_mesh::clamp_slot, rn_mesh::xyz_index;

constexpr int32_t MAX_ITERATIONS = 10000;

// ---- the workspace: ring [3 nf][2] i32 | scratch [nv][3] f32, rounded up to 8 bytes ----
constexpr int64_t ring_bytes(int64_t nf) { return 24 * nf; }
constexpr int64_t scratch_offset(int64_t nf) { return ring_bytes(nf); }     // a multiple of 8
constexpr int64_t workspace_bytes(int64_t nv, int64_t nf) {
    return (ring_bytes(nf) + 12 * nv + 7) / 8 * 8;
}

// rn_mesh_smooth.  The scalars first, then nv == 0 (nothing to write: EMPTY, whatever the
// pointers), then the pointers: faces and corners are read only where there are faces; `fixed`
// may be null and is not looked at here.
inline Verdict smooth_args(bool have_ctx, int64_t nv, const void *vertices_in, int64_t nf,
                           const void *faces, const void *offsets, const void *corners,
                           int32_t iterations, double lambda, double mu, double max_move,
                           const void *workspace, const void *vertices_out) {
    if (!have_ctx || !sizes_ok(nv, nf)) return INVALID;
    if (iterations < 0 || iterations > MAX_ITERATIONS) return INVALID;
    if (!std::isfinite(lambda) || !(lambda > 0.0) || !(lambda <= 1.0)) return INVALID;
    if (!std::isfinite(mu) || !(mu >= -1.0) || !(mu <= 0.0)) return INVALID;
    if (!(max_move > 0.0)) return INVALID;                  // (a NaN fails the test; +inf passes)
    if (nv == 0) return EMPTY;
    if (!vertices_in || !offsets || !vertices_out || !workspace) return INVALID;
    if (nf > 0 && (!faces || !corners)) return INVALID;
    if ((uintptr_t)workspace % 8 != 0) return INVALID;
    if (vertices_out == vertices_in || vertices_out == workspace || vertices_in == workspace)
        return INVALID;
    return LAUNCH;
}

// ---- the sequence of steps: 1 .. step_count, ping-pong so that the last one writes `out` ----
constexpr int64_t step_count(int32_t iterations, double mu) {
    return (int64_t)iterations * (mu != 0.0 ? 2 : 1);
}
// the factor of step i: lambda, then mu where there is one
constexpr double step_factor(int64_t i, double lambda, double mu) {
    return mu != 0.0 && i % 2 == 0 ? mu : lambda;
}
// step i of L writes `out` iff L - i is even, the scratch else; it reads what step i - 1 wrote,
// the first one `in`
constexpr bool step_writes_out(int64_t i, int64_t L) { return (L - i) % 2 == 0; }
constexpr float *step_target(int64_t i, int64_t L, float *scratch, float *out) {
    return step_writes_out(i, L) ? out : scratch;
}
constexpr const float *step_source(int64_t i, int64_t L, const float *in, float *scratch,
                                   float *out) {
    return i == 1 ? in : step_target(i - 1, L, scratch, out);
}

// ---- what the kernels address the ring with (the mesh: rn_mesh's guards) ----
constexpr size_t ring_index(int64_t k, int which) { return 2 * (size_t)k + (size_t)which; }

// ---- the ring entry of table position k in [0, 3 nf): the two other vertices of the face of
// corners[k], in the face's order after that corner; (-1, -1) for a corner outside [0, 3 nf) or a
// face with an index outside [0, nv) ----
constexpr void ring_entry(int64_t k, int64_t nv, int64_t nf, const int32_t *faces,
                          const int32_t *corners, int32_t *ring) {
    int32_t a = -1, b = -1;
    const int64_t c = corners[k];
    if (corner_in(c, nf)) {
        const int64_t f = c / 3;
        const int slot = (int)(c % 3);
        const int64_t i0 = faces[xyz_index(f, 0)], i1 = faces[xyz_index(f, 1)],
                      i2 = faces[xyz_index(f, 2)];
        if (vertex_in(i0, nv) && vertex_in(i1, nv) && vertex_in(i2, nv)) {
            a = faces[xyz_index(f, (slot + 1) % 3)];
            b = faces[xyz_index(f, (slot + 2) % 3)];
        }
    }
    ring[ring_index(k, 0)] = a;
    ring[ring_index(k, 1)] = b;
}

// the clamp of one coordinate to [start - max_move, start + max_move]; a NaN passes both tests
constexpr double clamped(double x, double start, double max_move) {
    const double lo = start - max_move, hi = start + max_move;
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return x;
}

// ---- one step of vertex v with factor t, from src to dst; `in` is what the clamp refers to.
// The ring holds -1 or vertices of [0, nv) (ring_entry wrote it); an entry outside is skipped all
// the same, so that no load depends on it ----
constexpr void step_vertex(int64_t v, int64_t nv, int64_t nf, const int32_t *offsets,
                           const int32_t *ring, const uint8_t *fixed, const float *in,
                           const float *src, double t, double max_move, float *dst) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t m = 0;
    const int64_t first = clamp_slot(offsets[v], nf), last = clamp_slot(offsets[v + 1], nf);
    for (int64_t k = first; k < last; k++) {
        const int64_t a = ring[ring_index(k, 0)], b = ring[ring_index(k, 1)];
        if (!vertex_in(a, nv) || !vertex_in(b, nv)) continue;
        sx = (sx + (double)src[xyz_index(a, 0)]) + (double)src[xyz_index(b, 0)];
        sy = (sy + (double)src[xyz_index(a, 1)]) + (double)src[xyz_index(b, 1)];
        sz = (sz + (double)src[xyz_index(a, 2)]) + (double)src[xyz_index(b, 2)];
        m = m + 2;
    }
    if (m == 0 || (fixed && fixed[v])) {
        dst[xyz_index(v, 0)] = src[xyz_index(v, 0)];
        dst[xyz_index(v, 1)] = src[xyz_index(v, 1)];
        dst[xyz_index(v, 2)] = src[xyz_index(v, 2)];
        return;
    }
    const double n = (double)m;
    const double px = (double)src[xyz_index(v, 0)], py = (double)src[xyz_index(v, 1)],
                 pz = (double)src[xyz_index(v, 2)];
    const double x = px + t * (sx / n - px), y = py + t * (sy / n - py),
                 z = pz + t * (sz / n - pz);
    dst[xyz_index(v, 0)] = (float)clamped(x, (double)in[xyz_index(v, 0)], max_move);
    dst[xyz_index(v, 1)] = (float)clamped(y, (double)in[xyz_index(v, 1)], max_move);
    dst[xyz_index(v, 2)] = (float)clamped(z, (double)in[xyz_index(v, 2)], max_move);
}

}  // namespace rn_sm
