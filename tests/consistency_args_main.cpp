// Stand-alone host program over raynet_amd/csrc/raynet_consistency_args.h: the refusals of
// rn_points_consistency and its accepted edges, the index arithmetic the kernel finds its point
// and addresses the arrays with, and the verdict of one view on one point at the bounds of its
// band -- which hold no HIP and so run here without a GPU.  tests/test_consistency_cpu.py builds it
// with -fsanitize=address,undefined and runs it; it exits 0 when every expectation holds and prints
// the first one that does not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_consistency_args.h"
#include "host_main.h"

using namespace rn_consistency;

// what the entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

int main() {
    unsigned char buffer[16] = {0};
    const void *p = buffer;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity();
    const double tiny = std::numeric_limits<double>::denorm_min();
    const double huge = std::numeric_limits<double>::max();
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();

    auto args = [&](int64_t n, int32_t V, int32_t H, int32_t W, int32_t exclude, double tol_abs,
                    double tol_rel, double border) {
        return points_args(true, n, p, V, p, H, W, p, exclude, tol_abs, tol_rel, border, p, p, p, p);
    };
    EXPECT(args(768, 3, 24, 32, 0, 0.08, 0.01, 2.5) == LAUNCH);
    // ---- the accepted edges
    EXPECT(args(1, 1, 1, 1, -1, 0.0, 0.0, 0.0) == LAUNCH);
    EXPECT(args(1, 1, 1, 1, 0, 0.0, 0.0, 0.0) == LAUNCH);                // the only view skipped
    EXPECT(args(1, 32, 1, 1, 31, 0.0, 0.0, 0.0) == LAUNCH);
    EXPECT(args(1, 32, 1, 1, -1, -0.0, -0.0, -0.0) == LAUNCH);           // -0 is 0
    EXPECT(args(MAX_POINTS, 3, imax, imax, 2, huge, huge, 1e300) == LAUNCH);
    EXPECT(args(1, 3, 24, 32, 0, tiny, tiny, tiny) == LAUNCH);
    // n == 0: nothing to write, whatever the pointers -- but the scalars are still checked
    EXPECT(args(0, 3, 24, 32, 0, 0.08, 0.01, 0.0) == EMPTY);
    EXPECT(points_args(true, 0, nullptr, 3, nullptr, 24, 32, nullptr, 0, 0.08, 0.01, 0.0, nullptr,
                       nullptr, nullptr, nullptr) == EMPTY);
    EXPECT(status(args(0, 3, 24, 32, 0, 0.08, 0.01, 0.0)) == RN_OK);
    EXPECT(status(args(0, 0, 24, 32, -1, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(0, 3, 24, 32, 3, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(0, 3, 24, 32, 0, nan, 0.01, 0.0)) == RN_ERR_INVALID);
    // ---- every refusal
    EXPECT(status(points_args(false, 768, p, 3, p, 24, 32, p, 0, 0.08, 0.01, 0.0, p, p, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(args(-1, 3, 24, 32, 0, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(std::numeric_limits<int64_t>::min(), 3, 24, 32, 0, 0.08, 0.01, 0.0)) ==
           RN_ERR_INVALID);
    EXPECT(status(args(MAX_POINTS + 1, 3, 24, 32, 0, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(std::numeric_limits<int64_t>::max(), 3, 24, 32, 0, 0.08, 0.01, 0.0)) ==
           RN_ERR_INVALID);
    for (int32_t V : {0, -1, 33, imax, imin})
        EXPECT(status(args(768, V, 24, 32, -1, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    for (int32_t bad : {0, -24, imin}) {
        EXPECT(status(args(768, 3, bad, 32, 0, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
        EXPECT(status(args(768, 3, 24, bad, 0, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    }
    for (int32_t exclude : {-2, 3, 4, imax, imin})
        EXPECT(status(args(768, 3, 24, 32, exclude, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    EXPECT(status(args(768, 32, 24, 32, 32, 0.08, 0.01, 0.0)) == RN_ERR_INVALID);
    for (double bad : {-tiny, -1.0, nan, inf, -inf}) {
        EXPECT(status(args(768, 3, 24, 32, 0, bad, 0.01, 0.0)) == RN_ERR_INVALID);
        EXPECT(status(args(768, 3, 24, 32, 0, 0.08, bad, 0.0)) == RN_ERR_INVALID);
        EXPECT(status(args(768, 3, 24, 32, 0, 0.08, 0.01, bad)) == RN_ERR_INVALID);
    }
    // every pointer on its own: all seven are read or written
    for (int k = 0; k < 7; k++) {
        const void *q[7] = {p, p, p, p, p, p, p};
        q[k] = nullptr;
        EXPECT(status(points_args(true, 768, q[0], 3, q[1], 24, 32, q[2], 0, 0.08, 0.01, 0.0, q[3],
                                  q[4], q[5], q[6])) == RN_ERR_INVALID);
    }

    // ---- point -> block and the three streams: a small table exhaustively, every entry inside
    {
        const int64_t n = 527;
        EXPECT(blocks(n, 256) == 3 && blocks(256, 256) == 1 && blocks(257, 256) == 2 &&
               blocks(1, 256) == 1 && blocks(0, 256) == 0);
        std::vector<double> coords((size_t)(3 * n), 1.0);
        std::vector<int> out((size_t)n, 0);
        double touched = 0.0;
        for (int64_t i = -3; i < blocks(n, 256) * 256 + 3; i++) {
            if (!point_in(i, n)) continue;
            for (int k = 0; k < 3; k++) touched += coords[coord_index(k, i, n)];
            out[(size_t)i]++;
        }
        EXPECT(touched == 3.0 * (double)n);
        for (int o : out) EXPECT(o == 1);
        EXPECT(!point_in(-1, n) && !point_in(n, n) && point_in(0, n) && point_in(n - 1, n));
        EXPECT(coord_index(0, 0, n) == 0 && coord_index(1, 0, n) == (size_t)n &&
               coord_index(2, n - 1, n) == (size_t)(3 * n - 1));
    }
    // the largest table: no overflow on the way, the block count fits the launch's 32 bits
    EXPECT(coord_index(2, MAX_POINTS - 1, MAX_POINTS) == 3ULL * (1ULL << 38) - 1);
    EXPECT(blocks(MAX_POINTS, 256) == ((int64_t)1 << 30));
    EXPECT(point_in(MAX_POINTS - 1, MAX_POINTS) && !point_in(MAX_POINTS, MAX_POINTS));
    EXPECT(!point_in(std::numeric_limits<int64_t>::min(), 5) &&
           !point_in(std::numeric_limits<int64_t>::max(), 5));

    // ---- the maps: the last pixel of the last view, and pixel 0 for what is not in view
    {
        const int V = 32, H = 5, W = 7;
        std::vector<float> depths(map_extent(V, H, W), 2.0f);
        EXPECT(depths.size() == (size_t)V * H * W);
        EXPECT(map_index(V - 1, H - 1, W - 1, H, W) == depths.size() - 1);
        double sum = 0.0;
        for (int v = 0; v < V; v++)
            for (int y = -2; y < H + 2; y++)
                for (int x = -2; x < W + 2; x++)
                    sum += depths[map_index(v, pixel_in(y, H) ? y : 0, pixel_in(x, W) ? x : 0, H, W)];
        EXPECT(sum == 2.0 * V * (H + 4) * (W + 4));
        EXPECT(!pixel_in(imin, H) && !pixel_in(imax, H) && !pixel_in(-1, H) && !pixel_in(H, H));
        EXPECT(map_extent(0, H, W) == 0);
        EXPECT(map_index(31, 46340, 46340, 46341, 46341) == 32ULL * 46341 * 46341 - 1);
        EXPECT(MAX_VIEWS == 32 && CAMERA_DOUBLES == 15);
    }

    // ---- one view's verdict.  zm = 2, dd = 1: s = (4 - 1) / 4 = 0.75; dd = 9: s = -1.25
    {
        const Vote at = classify(true, 2.0, 1.0, 0.75, 0.0);
        EXPECT(at.measured && at.agrees && !at.violates && at.s == 0.75);           // s == t
        const Vote past = classify(true, 2.0, 1.0, std::nextafter(0.75, 0.0), 0.0);
        EXPECT(past.measured && !past.agrees && past.violates);
        const Vote rel = classify(true, 2.0, 1.0, 0.0, 0.375);                      // t = 0.375 * 2
        EXPECT(rel.agrees && !rel.violates);
        const Vote both = classify(true, 2.0, 1.0, 0.25, 0.25);                     // 0.25 + 0.5
        EXPECT(both.agrees && !both.violates);
        const Vote low = classify(true, 2.0, 9.0, 1.25, 0.0);
        EXPECT(low.measured && low.agrees && !low.violates && low.s == -1.25);      // s == -t
        const Vote occluded = classify(true, 2.0, 9.0, std::nextafter(1.25, 0.0), 0.0);
        EXPECT(occluded.measured && !occluded.agrees && !occluded.violates);
        const Vote exact = classify(true, 5.0, 25.0, 0.0, 0.0);
        EXPECT(exact.agrees && !exact.violates && exact.s == 0.0);
        // what measures nothing: not in view, and a depth of 0, below 0, NaN, +inf
        const Vote out = classify(false, 2.0, 1.0, 0.75, 0.0);
        EXPECT(!out.measured && !out.agrees && !out.violates);
        for (double zm : {0.0, -0.0, -2.0, nan, inf, -inf}) {
            const Vote v = classify(true, zm, 1.0, 1e300, 1e300);
            EXPECT(!v.measured && !v.agrees && !v.violates);
        }
        // a NaN distance (a NaN point) measures but neither agrees nor violates -- the kernel
        // never asks: such a point is in no view
        const Vote nn = classify(true, 2.0, nan, 0.75, 0.0);
        EXPECT(nn.measured && !nn.agrees && !nn.violates);
        // the smallest and the largest depths: s stays comparable
        const Vote small = classify(true, (double)std::numeric_limits<float>::denorm_min(), 1.0, 0.0, 0.0);
        EXPECT(small.measured && !small.agrees && !small.violates);                 // far behind
        const Vote large = classify(true, (double)std::numeric_limits<float>::max(), 1.0, 0.0, 0.0);
        EXPECT(large.measured && !large.agrees && large.violates);
    }
    return finish("consistency");
}
