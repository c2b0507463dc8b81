// raynet_components_args.h -- the argument checks, the launch geometry and the union-find of
// rn_mesh_components (raynet_components.inl), host-only and free of HIP so that they compile into
// a stand-alone program (tests/components_args_main.cpp, built with the address and
// undefined-behaviour sanitizers and once more with the thread sanitizer by
// tests/test_components_cpu.py).  The launcher acts on the verdict; the kernels decide which faces
// count, size their grids and unite / find with the functions below and the guards of
// raynet_mesh_args.h.
//
// The union-find is a template over an atomics policy A with
//     int32_t A::load(int32_t x) const                          parent[x], a relaxed atomic load
//     int32_t A::cas(int32_t x, int32_t expect, int32_t v) const  compare-and-swap on parent[x],
//                                                               returns the value it found
//     void    A::store(int32_t x, int32_t v) const              parent[x] = v, a relaxed atomic store
//                                                               (flatten only, in a launch of its own)
// which the device instantiates with the agent-scope builtins and the host program with the
// __atomic builtins on plain int32_t.  The functions are constexpr only so that the device may call
// them; nothing here is evaluated at compile time.
//
// The invariant: parent[x] <= x at all times.  While faces are hooked the
// only writes are compare-and-swaps that replace a value by a strictly smaller one -- the hook
// parent[hi] = lo < hi on a root hi, and the path halving parent[x] = grandparent < parent; the
// launch after that stores the root of x, the smallest ancestor there is.  Every value a word ever
// holds is therefore an ancestor of x (or x), no cycle can form, and every chase follows strictly
// decreasing indices: at most nv steps.  No loop waits for another thread; the bounds below are a
// belt against a bug, not a part of the algorithm.
#pragma once

#include <cstddef>
#include <cstdint>

#include "raynet_mesh_args.h"

namespace rn_cc {

using rn_mesh::Verdict, rn_mesh::INVALID, rn_mesh::EMPTY, rn_mesh::LAUNCH;
using rn_mesh::INT32_LIMIT, rn_mesh::MAX_BLOCKS, rn_mesh::sizes_ok, rn_mesh::blocks;
using rn_mesh::vertex_in, rn_mesh::xyz_index;

// rn_mesh_components.  The scalars first, then nv == 0 (nothing to write: EMPTY, whatever the
// pointers), then the pointers: faces is read only where there are faces; the counts and the
// status word are optional.
inline Verdict components_args(bool have_ctx, int64_t nv, int64_t nf, const void *faces,
                               const void *labels) {
    if (!have_ctx || !sizes_ok(nv, nf)) return INVALID;
    if (nv == 0) return EMPTY;
    if (!labels) return INVALID;
    if (nf > 0 && !faces) return INVALID;
    return LAUNCH;
}

// ---- what the kernels guard, address and size their grids with: rn_mesh's, and ----
// a face counts (connects its vertices, is counted) iff all three indices name vertices
constexpr bool face_counts_in(int64_t nv, int64_t a, int64_t b, int64_t c) {
    return rn_mesh::face_names_vertices(nv, a, b, c);
}
constexpr size_t face_index(int64_t f, int slot) { return xyz_index(f, slot); }
// the hard bound of every chase and every retry loop
constexpr int64_t step_bound(int64_t nv) { return nv + 1; }

// ---- the union-find ----
// The root of x as far as this thread can see: the first ancestor r with parent[r] == r.  Halves
// the path on the way (parent[x]: p -> parent[p], by compare-and-swap, so only ever downwards).
// *ok = false when the chase is longer than `bound` steps, which the invariant rules out.
template <class A>
constexpr int32_t find(const A &at, int32_t x, int64_t bound, bool *ok) {
    int32_t p = at.load(x);
    for (int64_t step = 0; p != x; step++) {
        if (step >= bound) {
            *ok = false;
            return x;
        }
        const int32_t g = at.load(p);
        if (g != p) at.cas(x, p, g);                // g < p < x
        x = p;
        p = g;
    }
    return x;
}

// Joins the sets of a and b: finds both roots and hangs the larger under the smaller with
// CAS(&parent[hi], hi, lo).  A failed CAS means another thread hooked hi in the meantime -- its
// progress, not a wait -- and the search carries on from the value the CAS returned.  Returns
// false when a bound was reached.
template <class A>
constexpr bool unite(const A &at, int32_t a, int32_t b, int64_t bound) {
    bool ok = true;
    for (int64_t tries = 0; tries < bound; tries++) {
        a = find(at, a, bound, &ok);
        b = find(at, b, bound, &ok);
        if (!ok) return false;
        if (a == b) return true;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t seen = at.cas(hi, hi, lo);
        if (seen == hi) return true;
        a = seen;                                   // an ancestor of hi, below it
        b = lo;
    }
    return false;
}

// The launch after the hooks: parent[v] = the root of v.  Other threads chase through the same
// words meanwhile; the only value this puts into a word is a root, an ancestor of its vertex, and
// roots do not change in this launch, so a chase that meets it is merely shorter.  No halving: one
// store per vertex.  Returns false when the chase is longer than `bound` steps.
template <class A>
constexpr bool flatten(const A &at, int32_t v, int64_t bound) {
    int32_t x = v, p = at.load(x);
    for (int64_t step = 0; p != x; step++) {
        if (step >= bound) return false;
        x = p;
        p = at.load(x);
    }
    at.store(v, x);
    return true;
}

}  // namespace rn_cc
