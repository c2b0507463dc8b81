// Stand-alone host program over raynet_amd/csrc/raynet_volume_args.h: the argument checks and the
// output addressing of rn_occupancy_grid / rn_volume_render, which hold no HIP and so run here
// without a GPU.  tests/test_volume_args.py builds it with -fsanitize=address,undefined and runs
// it; it exits 0 when every expectation holds and prints the first one that does not.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_volume_args.h"
#include "host_main.h"

using namespace rn_volume;

// what an entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

int main() {
    float a[3] = {0, 0, 0};
    const void *p = a;
    // rn_volume_render: an empty launch is RN_OK whatever the pointers are, and launches nothing
    EXPECT(render_args(true, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == EMPTY);
    EXPECT(status(render_args(true, 0, nullptr, nullptr, nullptr, nullptr, nullptr, -5)) == RN_OK);
    // ... but not without a context, and never for a negative count
    EXPECT(status(render_args(false, 0, p, p, p, p, p, 0)) == RN_ERR_INVALID);
    EXPECT(status(render_args(true, -1, p, p, p, p, p, 10)) == RN_ERR_INVALID);
    // a plane stride shorter than the rays
    EXPECT(status(render_args(true, 8, p, p, p, p, p, 7)) == RN_ERR_INVALID);
    EXPECT(status(render_args(true, 8, p, p, p, p, p, -1)) == RN_ERR_INVALID);
    EXPECT(render_args(true, 8, p, p, p, p, p, 8) == LAUNCH);
    EXPECT(render_args(true, 0x7fffffff, p, p, p, p, p, 0x7fffffffLL) == LAUNCH);
    // every pointer on its own
    for (int k = 0; k < 5; k++) {
        const void *q[5] = {p, p, p, p, p};
        q[k] = nullptr;
        EXPECT(status(render_args(true, 8, q[0], q[1], q[2], q[3], q[4], 8)) == RN_ERR_INVALID);
    }
    // rn_occupancy_grid
    EXPECT(grid_args(true, p, 0, p) == LAUNCH && grid_args(true, p, 1, p) == LAUNCH);
    EXPECT(status(grid_args(false, p, 0, p)) == RN_ERR_INVALID);
    EXPECT(status(grid_args(true, nullptr, 0, p)) == RN_ERR_INVALID);
    EXPECT(status(grid_args(true, p, 0, nullptr)) == RN_ERR_INVALID);
    EXPECT(status(grid_args(true, p, 2, p)) == RN_ERR_INVALID);
    EXPECT(status(grid_args(true, p, -1, p)) == RN_ERR_INVALID);

    // the output addressing: a heap array of exactly out_extent floats takes every write of n
    // rays at a stride of n + 5 (the address sanitizer watches the ends) and the gaps stay as
    // they were
    const int32_t n = 197;
    const int64_t stride = n + 5;
    EXPECT(out_extent(0, stride) == 0);
    EXPECT(out_extent(n, stride) == (size_t)(4 * stride + n));
    std::vector<float> out(out_extent(n, stride), -7.0f);
    for (int plane = 0; plane < PLANES; plane++)
        for (int32_t r = 0; r < n; r++) out[out_index(plane, stride, r)] = (float)plane;
    for (int plane = 0; plane < PLANES; plane++) {
        EXPECT(out[out_index(plane, stride, 0)] == (float)plane);
        EXPECT(out[out_index(plane, stride, n - 1)] == (float)plane);
        if (plane < PLANES - 1)
            for (int64_t g = n; g < stride; g++) EXPECT(out[(size_t)plane * stride + g] == -7.0f);
    }
    // no 32-bit overflow in between: the last float of 2^31 - 1 rays at the same stride
    EXPECT(out_index(4, 0x7fffffffLL, 0x7ffffffe) == (size_t)4 * 0x7fffffffULL + 0x7ffffffeULL);
    return finish("volume");
}
