// raynet_volume_args.h -- the argument checks and the output addressing of rn_occupancy_grid and
// rn_volume_render (raynet_volume.inl), host-only and free of HIP so that they compile into a
// stand-alone program (tests/volume_args_main.cpp, built with the address and undefined-behaviour
// sanitizers by tests/test_volume_args.py).  The launchers act on the verdict and do no pointer
// arithmetic of their own before it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rn_volume {

constexpr int PLANES = 5;        // depth | opacity | expected depth | confidence | median depth

enum Verdict { INVALID = -1, EMPTY = 0, LAUNCH = 1 };

// rn_volume_render: an empty launch (n == 0) is fine whatever the pointers are, as for every
// entry over n rays; anything else needs every pointer and a plane stride that holds n rays.
inline Verdict render_args(bool have_ctx, int32_t n, const void *ray_start, const void *ray_end,
                           const void *camera_center, const void *belief, const void *out,
                           int64_t out_stride) {
    if (!have_ctx || n < 0) return INVALID;
    if (n == 0) return EMPTY;
    if (!ray_start || !ray_end || !camera_center || !belief || !out) return INVALID;
    if (out_stride < (int64_t)n) return INVALID;
    return LAUNCH;
}

// rn_occupancy_grid: G = gx gy gz voxels, never empty for a context rn_create admitted
inline Verdict grid_args(bool have_ctx, const void *acc, int32_t bricked, const void *belief_out) {
    if (!have_ctx || !acc || !belief_out || (bricked != 0 && bricked != 1)) return INVALID;
    return LAUNCH;
}

// (constexpr: the kernel addresses its output with the same function)
// entry of ray `ray` in plane `plane` of an out array of `out_stride` floats per plane
constexpr size_t out_index(int plane, int64_t out_stride, int32_t ray) {
    return (size_t)plane * (size_t)out_stride + (size_t)ray;
}

// floats the kernel may touch in `out`: the last plane ends at its n-th entry, not at its stride
constexpr size_t out_extent(int32_t n, int64_t out_stride) {
    return n > 0 ? out_index(PLANES - 1, out_stride, n - 1) + 1 : 0;
}

}  // namespace rn_volume
