// raynet_mesh_args.h -- what the stages that read an indexed triangle mesh share: the limits of its
// sizes, the guards of its indices and the capped launch geometry.  These are the memory-safety
// contract of the mesh kernels, stated once; raynet_appearance_args.h, raynet_components_args.h,
// raynet_smooth_args.h and raynet_simplify_args.h import the names they use into their own
// namespace with using-declarations.  Host-only and free of HIP like them; the functions are
// constexpr only so that the device may call them.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rn_mesh {

constexpr int64_t INT32_LIMIT = ((int64_t)1 << 31) - 1;
constexpr int MAX_BLOCKS = 2048;        // the rest of a launch is a grid-stride loop

enum Verdict { INVALID = -1, EMPTY = 0, LAUNCH = 1 };

// the sizes of a mesh an entry takes
constexpr bool sizes_ok(int64_t nv, int64_t nf) {
    return nv >= 0 && nf >= 0 && nv <= INT32_LIMIT - 1      // a vertex and the bound nv + 1 (the
                                                            // entries of `offsets`) are int32
           && nf <= INT32_LIMIT / 3;                        // a corner 3 f + slot is an int32
}

// ---- what the kernels guard, address and size their grids with ----
constexpr bool vertex_in(int64_t v, int64_t nv) { return v >= 0 && v < nv; }
constexpr bool face_in(int64_t f, int64_t nf) { return f >= 0 && f < nf; }
// the corner c = 3 f + slot names an entry of `faces`
constexpr bool corner_in(int64_t c, int64_t nf) { return c >= 0 && c < 3 * nf; }
// the range [first, last) of a vertex's corners, cut to the entries `corners` has
constexpr int64_t clamp_slot(int64_t k, int64_t nf) { return k < 0 ? 0 : (k > 3 * nf ? 3 * nf : k); }
// A face counts iff all three of its indices name vertices.  (ring_entry, face_clusters and
// k_vertex_area_normals write the three tests out instead: there the compiler loads each index only
// once the one in front has passed, and through this function it loads all three first.)
constexpr bool face_names_vertices(int64_t nv, int64_t a, int64_t b, int64_t c) {
    return vertex_in(a, nv) && vertex_in(b, nv) && vertex_in(c, nv);
}
constexpr size_t xyz_index(int64_t row, int column) { return 3 * (size_t)row + (size_t)column; }
// blocks of `block` threads over n items, at most MAX_BLOCKS (and at least one)
constexpr int64_t blocks(int64_t n, int block) {
    const int64_t want = (n + block - 1) / block;
    return want < 1 ? 1 : (want > MAX_BLOCKS ? MAX_BLOCKS : want);
}

}  // namespace rn_mesh
