// Stand-alone host program over raynet_amd/csrc/raynet_fusion_args.h: the refusals of
// rn_tsdf_integrate and its accepted edges, and the index arithmetic the kernel finds its voxel
// and addresses the maps with, which hold no HIP and so run here without a GPU.
// tests/test_fusion_cpu.py builds it with -fsanitize=address,undefined and runs it; it exits 0
// when every expectation holds and prints the first one that does not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_fusion_args.h"
#include "host_main.h"

using namespace rn_fusion;

// what the entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

int main() {
    unsigned char buffer[16] = {0};
    const void *p = buffer;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity();
    const double tiny = std::numeric_limits<double>::denorm_min();

    auto args = [&](int32_t V, int32_t H, int32_t W, double trunc, double border) {
        return integrate_args(true, V, p, H, W, p, trunc, border, p, p);
    };
    EXPECT(args(5, 24, 32, 0.48, 1.5) == LAUNCH);
    // ---- the accepted edges
    EXPECT(args(0, 24, 32, 0.48, 0.0) == LAUNCH);                        // V == 0: all 1 / all 0
    EXPECT(integrate_args(true, 0, nullptr, 1, 1, nullptr, 0.48, 0.0, p, p) == LAUNCH);
    EXPECT(args(4096, 1, 1, 0.48, 0.0) == LAUNCH);
    EXPECT(args(1, 1, 1, tiny, 0.0) == LAUNCH);
    EXPECT(args(1, 1, 1, std::numeric_limits<double>::max(), 1e300) == LAUNCH);
    EXPECT(args(1, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::max(), 1.0,
                0.0) == LAUNCH);
    // ---- every refusal
    EXPECT(status(integrate_args(false, 5, p, 24, 32, p, 0.48, 0.0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(args(-1, 24, 32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(4097, 24, 32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(std::numeric_limits<int32_t>::max(), 24, 32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(std::numeric_limits<int32_t>::min(), 24, 32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 0, 32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 0, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, -24, 32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, -32, 0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(0, 0, 32, 0.48, 0.0)) == RN_ERR_INVALID);         // also without views
    EXPECT(status(args(5, 24, 32, 0.0, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, -0.0, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, -0.48, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, nan, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, inf, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, 0.48, -tiny)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, 0.48, -1.5)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, 0.48, nan)) == RN_ERR_INVALID);
    EXPECT(status(args(5, 24, 32, 0.48, inf)) == RN_ERR_INVALID);
    EXPECT(args(5, 24, 32, 0.48, -0.0) == LAUNCH);                       // -0 is 0
    // every required pointer on its own; weights is not among them
    EXPECT(status(integrate_args(true, 5, nullptr, 24, 32, p, 0.48, 0.0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(integrate_args(true, 5, p, 24, 32, nullptr, 0.48, 0.0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(integrate_args(true, 5, p, 24, 32, p, 0.48, 0.0, nullptr, p)) == RN_ERR_INVALID);
    EXPECT(status(integrate_args(true, 5, p, 24, 32, p, 0.48, 0.0, p, nullptr)) == RN_ERR_INVALID);
    EXPECT(status(integrate_args(true, 0, nullptr, 24, 32, nullptr, 0.48, 0.0, nullptr, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(integrate_args(true, 0, nullptr, 24, 32, nullptr, 0.48, 0.0, p, nullptr)) ==
           RN_ERR_INVALID);

    // ---- voxel <-> (i, j, k): a small grid exhaustively, every table entry inside its table
    const int32_t gx = 7, gy = 5, gz = 67;
    const int64_t G = voxels(gx, gy, gz);
    EXPECT(G == 7 * 5 * 67 && blocks(G, 256) == 10 && blocks(256, 256) == 1 && blocks(257, 256) == 2);
    std::vector<float> axes((size_t)(gx + gy + gz), 1.0f), out((size_t)G, 0.0f);
    double touched = 0.0;
    for (int64_t g = -3; g < blocks(G, 256) * 256 + 3; g++) {
        if (!voxel_in(g, G)) continue;
        const Voxel v = voxel_of(g, gy, gz);
        EXPECT(v.i >= 0 && v.i < gx && v.j >= 0 && v.j < gy && v.k >= 0 && v.k < gz);
        EXPECT(voxel_index(v.i, v.j, v.k, gy, gz) == g);
        touched += axes[(size_t)axis_x(v)] + axes[(size_t)axis_y(v, gx)] +
                   axes[(size_t)axis_z(v, gx, gy)];
        out[(size_t)g] += 1.0f;
    }
    EXPECT(touched == 3.0 * (double)G);
    for (float o : out) EXPECT(o == 1.0f);
    EXPECT(!voxel_in(-1, G) && !voxel_in(G, G) && voxel_in(0, G) && voxel_in(G - 1, G));
    {
        const Voxel v = voxel_of(G - 1, gy, gz);
        EXPECT(v.i == gx - 1 && v.j == gy - 1 && v.k == gz - 1);
        EXPECT(axis_z(v, gx, gy) == gx + gy + gz - 1);
    }
    // the largest grids rn_create admits: 1024 voxels an axis, fewer than 2^24 bricks of 4^3
    {
        const int32_t bx = 1024, by = 1024, bz = 1020;
        const int64_t B = voxels(bx, by, bz);
        EXPECT(B == (int64_t)1024 * 1024 * 1020 && B < ((int64_t)1 << 31));
        const Voxel v = voxel_of(B - 1, by, bz);
        EXPECT(v.i == 1023 && v.j == 1023 && v.k == 1019);
        EXPECT(voxel_index(1023, 1023, 1019, by, bz) == B - 1);
        EXPECT(blocks(B, 256) == (B + 255) / 256 && blocks(B, 256) < ((int64_t)1 << 32));
        // (the arithmetic itself is 64-bit: a grid beyond 2^31 voxels would index as well)
        const int64_t C = voxels(1024, 1024, 1024);
        EXPECT(C == ((int64_t)1 << 30));
        const int64_t big = voxels(2000, 2000, 2000);
        EXPECT(big == 8000000000LL);
        const Voxel w = voxel_of(big - 1, 2000, 2000);
        EXPECT(w.i == 1999 && w.j == 1999 && w.k == 1999);
        EXPECT(voxel_index(1999, 1999, 1999, 2000, 2000) == big - 1);
    }

    // ---- the maps: the last pixel of the last view, and pixel 0 for what is not in view
    const int V = 3, H = 5, W = 7;
    std::vector<float> depths(map_extent(V, H, W), 2.0f);
    EXPECT(depths.size() == (size_t)V * H * W);
    EXPECT(map_index(V - 1, H - 1, W - 1, H, W) == depths.size() - 1);
    EXPECT(map_index(0, 0, 0, H, W) == 0 && map_index(1, 0, 0, H, W) == (size_t)H * W);
    EXPECT(map_index(0, 1, 0, H, W) == (size_t)W && map_index(0, 0, 1, H, W) == 1);
    double sum = 0.0;
    for (int v = 0; v < V; v++)
        for (int y = -2; y < H + 2; y++)
            for (int x = -2; x < W + 2; x++)
                sum += depths[map_index(v, pixel_in(y, H) ? y : 0, pixel_in(x, W) ? x : 0, H, W)];
    EXPECT(sum == 2.0 * V * (H + 4) * (W + 4));
    EXPECT(!pixel_in(-1, H) && !pixel_in(H, H) && pixel_in(0, H) && pixel_in(H - 1, H));
    EXPECT(!pixel_in(std::numeric_limits<int>::min(), H) &&
           !pixel_in(std::numeric_limits<int>::max(), H));
    EXPECT(map_extent(0, H, W) == 0);
    // V H W beyond 2^31, and beyond 2^32: no overflow on the way
    EXPECT(map_index(8, 16383, 16383, 16384, 16384) == 9ULL * 16384 * 16384 - 1);
    EXPECT(9ULL * 16384 * 16384 > (1ULL << 31) && 9ULL * 16384 * 16384 < (1ULL << 32));
    EXPECT(map_index(4095, 4095, 4095, 4096, 4096) == 4096ULL * 4096 * 4096 - 1);
    EXPECT(map_extent(4096, 4096, 4096) == (1ULL << 36));
    EXPECT(map_index(4095, 46340, 46340, 46341, 46341) == 4096ULL * 46341 * 46341 - 1);
    EXPECT(MAX_VIEWS == 4096 && CAMERA_DOUBLES == 15);
    return finish("fusion");
}
