// Stand-alone host program over raynet_amd/csrc/raynet_overlap_args.h: the refusals of
// rn_view_overlap / rn_view_gain and their accepted edges, the launch geometry (the block cap, the
// tiles a block strides over, the bound of a block's uint32 counters), the index of a pair's
// counter, and the three predicates -- a view sees a point, two views share it, a point is short
// -- at the edges of their definitions; which hold no HIP and so run here without a GPU.
// tests/test_view_selection_cpu.py builds it with -fsanitize=address,undefined and runs it; it
// exits 0 when every expectation holds and prints the first one that does not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_overlap_args.h"
#include "host_main.h"

using namespace rn_overlap;

static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

// a camera at (cx, cy, height) looking straight down at the plane z = 0
static void plane_camera(double *row, double cx, double cy, double height, double focal, double u0,
                         double v0) {
    const double P[12] = {focal, 0.0, -u0, -focal * cx + u0 * height,
                          0.0, focal, -v0, -focal * cy + v0 * height,
                          0.0, 0.0, -1.0, height};
    for (int k = 0; k < 12; k++) row[k] = P[k];
    row[12] = cx, row[13] = cy, row[14] = height;
}

int main() {
    unsigned char buffer[16] = {0};
    const void *p = buffer;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity();
    const double tiny = std::numeric_limits<double>::denorm_min();
    const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
    const int64_t lmax = std::numeric_limits<int64_t>::max(), lmin = std::numeric_limits<int64_t>::min();

    // ---- rn_view_overlap
    auto args = [&](int64_t n, int32_t V, int32_t H, int32_t W, double tol, double min_cos,
                    double border, double cos_lo, double cos_hi) {
        return overlap_args(true, n, p, p, V, p, H, W, p, tol, min_cos, border, cos_lo, cos_hi, p, p);
    };
    EXPECT(args(1681, 8, 24, 32, 0.1, 0.2, 1.5, 0.7, 0.99) == LAUNCH);
    EXPECT(args(1, 1, 1, 1, 0.0, 0.0, 0.0, 0.0, 0.0) == LAUNCH);
    EXPECT(args(1, 64, 1, 1, -0.0, -0.0, -0.0, -0.0, 1.0) == LAUNCH);
    EXPECT(args(MAX_POINTS, 64, imax, imax, 1e300, 1e300, 1e300, 1.0, 1.0) == LAUNCH);
    EXPECT(args(1, 3, 24, 32, tiny, tiny, tiny, tiny, tiny) == LAUNCH);
    EXPECT(args(1, 3, 24, 32, 0.0, 0.0, 0.0, 0.5, 0.5) == LAUNCH);                // an empty band's edge
    // normals and depths may be NULL
    EXPECT(overlap_args(true, 5, p, nullptr, 3, p, 24, 32, nullptr, 0, 0, 0, 0.1, 0.9, p, p) == LAUNCH);
    // n == 0: nothing to write, whatever the pointers -- but the scalars are still checked
    EXPECT(args(0, 3, 24, 32, 0.0, 0.0, 0.0, 0.1, 0.9) == EMPTY);
    EXPECT(overlap_args(true, 0, nullptr, nullptr, 3, nullptr, 24, 32, nullptr, 0, 0, 0, 0.1, 0.9,
                        nullptr, nullptr) == EMPTY);
    EXPECT(status(args(0, 0, 24, 32, 0.0, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
    EXPECT(status(args(0, 3, 24, 32, nan, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
    EXPECT(status(args(0, 3, 24, 32, 0.0, 0.0, 0.0, 0.9, 0.1)) == RN_ERR_INVALID);
    // every refusal
    EXPECT(status(overlap_args(false, 5, p, p, 3, p, 24, 32, p, 0, 0, 0, 0.1, 0.9, p, p)) ==
           RN_ERR_INVALID);
    for (int64_t n : {(int64_t)-1, lmin, MAX_POINTS + 1, lmax})
        EXPECT(status(args(n, 3, 24, 32, 0.0, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
    for (int32_t V : {0, -1, 65, imax, imin})
        EXPECT(status(args(5, V, 24, 32, 0.0, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
    for (int32_t bad : {0, -24, imin}) {
        EXPECT(status(args(5, 3, bad, 32, 0.0, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
        EXPECT(status(args(5, 3, 24, bad, 0.0, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
    }
    for (double bad : {-tiny, -1.0, nan, inf, -inf}) {
        EXPECT(status(args(5, 3, 24, 32, bad, 0.0, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
        EXPECT(status(args(5, 3, 24, 32, 0.0, bad, 0.0, 0.1, 0.9)) == RN_ERR_INVALID);
        EXPECT(status(args(5, 3, 24, 32, 0.0, 0.0, bad, 0.1, 0.9)) == RN_ERR_INVALID);
        EXPECT(status(args(5, 3, 24, 32, 0.0, 0.0, 0.0, bad, 0.9)) == RN_ERR_INVALID);
        EXPECT(status(args(5, 3, 24, 32, 0.0, 0.0, 0.0, 0.1, bad)) == RN_ERR_INVALID);
    }
    EXPECT(status(args(5, 3, 24, 32, 0.0, 0.0, 0.0, 0.1, std::nextafter(1.0, 2.0))) == RN_ERR_INVALID);
    EXPECT(status(args(5, 3, 24, 32, 0.0, 0.0, 0.0, 0.5, std::nextafter(0.5, 0.0))) == RN_ERR_INVALID);
    // the four pointers that are always read or written, each on its own
    for (int k = 0; k < 4; k++) {
        const void *q[4] = {p, p, p, p};
        q[k] = nullptr;
        EXPECT(status(overlap_args(true, 5, q[0], p, 3, q[1], 24, 32, p, 0, 0, 0, 0.1, 0.9, q[2],
                                   q[3])) == RN_ERR_INVALID);
    }

    // ---- rn_view_gain
    EXPECT(gain_args(true, 5, p, 3, 1, p) == LAUNCH);
    EXPECT(gain_args(true, MAX_POINTS, p, 64, 64, p) == LAUNCH);
    EXPECT(gain_args(true, 1, p, 1, 1, p) == LAUNCH);
    EXPECT(gain_args(true, 0, nullptr, 3, 1, nullptr) == EMPTY);
    EXPECT(gain_args(true, 0, nullptr, 0, 1, nullptr) == INVALID);
    EXPECT(gain_args(false, 5, p, 3, 1, p) == INVALID);
    for (int64_t n : {(int64_t)-1, lmin, MAX_POINTS + 1, lmax}) EXPECT(gain_args(true, n, p, 3, 1, p) == INVALID);
    for (int32_t bad : {0, -1, 65, imax, imin}) {
        EXPECT(gain_args(true, 5, p, bad, 1, p) == INVALID);
        EXPECT(gain_args(true, 5, p, 3, bad, p) == INVALID);
    }
    EXPECT(gain_args(true, 5, nullptr, 3, 1, p) == INVALID);
    EXPECT(gain_args(true, 5, p, 3, 1, nullptr) == INVALID);

    // ---- the launch: every point in exactly one (block, round, lane), the cap, the counters' bound
    EXPECT(BLOCK_SIZE == 256 && MAX_BLOCKS == 1024 && MAX_VIEWS == 64 && MAX_PAIRS == 2080);
    EXPECT(tiles(0) == 0 && tiles(1) == 1 && tiles(256) == 1 && tiles(257) == 2);
    EXPECT(blocks(0) == 0 && blocks(1) == 1 && blocks(257) == 2);
    EXPECT(blocks((int64_t)MAX_BLOCKS * BLOCK_SIZE) == MAX_BLOCKS);
    EXPECT(blocks((int64_t)MAX_BLOCKS * BLOCK_SIZE + 1) == MAX_BLOCKS);
    EXPECT(tiles((int64_t)MAX_BLOCKS * BLOCK_SIZE + 1) == MAX_BLOCKS + 1);
    EXPECT(blocks(MAX_POINTS) == MAX_BLOCKS && tiles(MAX_POINTS) == ((int64_t)1 << 30));
    EXPECT(block_points_max(MAX_POINTS) == ((int64_t)1 << 28));
    EXPECT(block_points_max(MAX_POINTS) <= (int64_t)std::numeric_limits<uint32_t>::max());
    EXPECT(block_points_max(1) == 256 && block_points_max(0) == 0);
    EXPECT(block_points_max((int64_t)MAX_BLOCKS * BLOCK_SIZE + 1) == 512);
    for (int64_t n : {(int64_t)1, (int64_t)255, (int64_t)257, (int64_t)1000,
                      (int64_t)MAX_BLOCKS * BLOCK_SIZE + 1, (int64_t)3 * MAX_BLOCKS * BLOCK_SIZE - 7}) {
        std::vector<unsigned char> met((size_t)n, 0);
        int64_t most = 0;
        for (int64_t b = 0; b < blocks(n); b++) {
            int64_t mine = 0;
            for (int64_t tile = b; tile < tiles(n); tile += blocks(n))
                for (int lane = 0; lane < BLOCK_SIZE; lane++) {
                    const int64_t i = tile * BLOCK_SIZE + lane;
                    mine++;
                    if (point_in(i, n)) met[(size_t)i]++;
                }
            most = std::max(most, mine);
        }
        bool once = true;
        for (unsigned char m : met) once = once && m == 1;
        EXPECT(once);
        EXPECT(most == block_points_max(n));
    }
    EXPECT(!point_in(-1, 5) && !point_in(5, 5) && point_in(0, 5) && point_in(4, 5));
    EXPECT(!point_in(lmin, 5) && !point_in(lmax, 5));
    EXPECT(coord_index(2, MAX_POINTS - 1, MAX_POINTS) == 3ULL * (1ULL << 38) - 1);
    EXPECT(coord_index(1, 0, 7) == 7);

    // ---- the pairs' counters: the upper triangle row by row, every index once, the last one last
    for (int V : {1, 2, 3, 33, 64}) {
        std::vector<int> hit((size_t)pair_count(V), 0);
        int next = 0;
        bool in_order = true;
        for (int i = 0; i < V; i++)
            for (int j = i; j < V; j++) {
                in_order = in_order && pair_index(i, j, V) == next++;
                hit[(size_t)pair_index(i, j, V)]++;
            }
        EXPECT(in_order && next == pair_count(V));
        for (int h : hit) EXPECT(h == 1);
        EXPECT(pair_index(V - 1, V - 1, V) == pair_count(V) - 1);
        EXPECT(matrix_index(V - 1, V - 1, V) == (size_t)V * V - 1);
    }
    EXPECT(pair_count(64) == MAX_PAIRS);
    EXPECT(low_bits(1) == 1 && low_bits(3) == 7 && low_bits(63) == 0x7FFFFFFFFFFFFFFFULL &&
           low_bits(64) == 0xFFFFFFFFFFFFFFFFULL);

    // ---- sharing: the two exact cases of the band
    {
        // centres (1, 0, 1) and (0, 1, 1), the point at the origin: dot = 1, q = 4, cosine 1/2
        double rows[2 * 15];
        plane_camera(rows, 1.0, 0.0, 1.0, 8.0, 15.5, 11.5);
        plane_camera(rows + 15, 0.0, 1.0, 1.0, 8.0, 15.5, 11.5);
        const ToCentre a = to_centre(rows, 0, 0.0, 0.0, 0.0), b = to_centre(rows, 1, 0.0, 0.0, 0.0);
        EXPECT(a.dd == 2.0 && b.dd == 2.0 && a.dx == 1.0 && b.dy == 1.0);
        auto band = [&](double lo, double hi) { return shares(a, b, lo * lo, hi * hi); };
        EXPECT(band(0.5, 1.0) && !band(std::nextafter(0.5, 1.0), 1.0));
        EXPECT(band(0.0, 0.5) && !band(0.0, std::nextafter(0.5, 0.0)));
        EXPECT(band(0.5, 0.5));
        // both cameras see the origin at 24 x 32, and to_centre has project's bits
        for (int v = 0; v < 2; v++) {
            const Sight s = sees(rows, v, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 24, 32, nullptr,
                                 0.0, 0.0, 31.0, 23.0);
            const ToCentre c = to_centre(rows, v, 0.0, 0.0, 0.0);
            EXPECT(s.ok && s.dx == c.dx && s.dy == c.dy && s.dz == c.dz && s.dd == c.dd);
        }
        // centres (0, 0, 4) and (3, 0, 4): 4/5 in exact arithmetic, but 0.8 * 0.8 * 400 > 256
        plane_camera(rows, 0.0, 0.0, 4.0, 8.0, 15.5, 11.5);
        plane_camera(rows + 15, 3.0, 0.0, 4.0, 8.0, 15.5, 11.5);
        const ToCentre c = to_centre(rows, 0, 0.0, 0.0, 0.0), d = to_centre(rows, 1, 0.0, 0.0, 0.0);
        EXPECT(c.dd == 16.0 && d.dd == 25.0);
        EXPECT(0.8 * 0.8 * 400.0 > 256.0);
        EXPECT(!shares(c, d, 0.8 * 0.8, 1.0));
        EXPECT(shares(c, d, std::nextafter(0.8, 0.0) * std::nextafter(0.8, 0.0), 1.0));
        // a right angle and an obtuse one never count: dot > 0 is strict
        plane_camera(rows, 1.0, 0.0, 0.0, 8.0, 15.5, 11.5);
        plane_camera(rows + 15, 0.0, 1.0, 0.0, 8.0, 15.5, 11.5);
        EXPECT(!shares(to_centre(rows, 0, 0, 0, 0), to_centre(rows, 1, 0, 0, 0), 0.0, 1.0));
        // a NaN point shares nothing
        EXPECT(!shares(to_centre(rows, 0, nan, 0, 0), to_centre(rows, 1, nan, 0, 0), 0.0, 1.0));
    }

    // ---- seeing: facing, occlusion at the nearest pixel, pixel (0, 0) for what does not count
    {
        const int H = 24, W = 32;
        double row[15];
        plane_camera(row, 0.0, 0.0, 4.0, 16.0, 8.0, 8.0);       // (x, y, 0) lands at (4 x + 8, 4 y + 8)
        std::vector<float> maps((size_t)H * W, 4.0f);
        auto depths = exact(maps);
        auto see = [&](double x, double y, double z, double nx, double ny, double nz, double min_cos,
                       const float *dm, double tol, double border) {
            const double nn = (nx * nx + ny * ny) + nz * nz;
            return sees(row, 0, x, y, z, nx, ny, nz, nn, min_cos * min_cos, H, W, dm, tol, border,
                        (double)(W - 1) - border, (double)(H - 1) - border).ok;
        };
        EXPECT(see(0, 0, 0, 0, 0, 0, 0.0, nullptr, 0.0, 0.0));
        EXPECT(see(0, 0, 0, 0, 0, 2, 0.0, nullptr, 0.0, 0.0));              // facing
        EXPECT(!see(0, 0, 0, 0, 0, -1, 0.0, nullptr, 0.0, 0.0));            // facing away
        EXPECT(!see(0, 0, 0, 1, 0, 0, 0.0, nullptr, 0.0, 0.0));             // perpendicular: strict
        EXPECT(see(0, 0, 0, 0, 0, 1, 0.99, nullptr, 0.0, 0.0) && !see(0, 0, 0, 0, 0, 1, 1.0, nullptr, 0.0, 0.0));
        EXPECT(see(0, 0, 0, 0, 0, 0, 0.0, depths.get(), 0.0, 0.0));         // dd = 16 <= 4^2
        depths[(size_t)8 * W + 8] = 3.0f;
        EXPECT(!see(0, 0, 0, 0, 0, 0, 0.0, depths.get(), 0.0, 0.0));        // behind the occluder
        EXPECT(see(0, 0, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 0.0));         // ... within tol
        // (3 + tol must round below 4: one step below 1 would round back up to it)
        EXPECT(!see(0, 0, 0, 0, 0, 0, 0.0, depths.get(), std::nextafter(4.0, 0.0) - 3.0, 0.0));
        for (float none : {0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN()}) {
            depths[(size_t)8 * W + 8] = none;
            EXPECT(!see(0, 0, 0, 0, 0, 0, 0.0, depths.get(), 100.0, 0.0));
        }
        depths[(size_t)8 * W + 8] = std::numeric_limits<float>::infinity();
        EXPECT(see(0, 0, 0, 0, 0, 0, 0.0, depths.get(), 0.0, 0.0));
        // halves go to the even pixel: X = 0.5 reads column 0, X = 1.5 column 2
        depths[(size_t)8 * W + 1] = 0.0f;
        EXPECT(see(-1.875, 0, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 0.0));
        EXPECT(see(-1.625, 0, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 0.0));
        // the border, on it and one step outside; what is out of view reads pixel (0, 0) (the
        // exactly sized map would fault otherwise)
        EXPECT(see(-2, 0, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 0.0) && !see(-2, 0, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 2.5));
        EXPECT(!see(std::nextafter(-2.0, -inf), 0, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 0.0));
        EXPECT(!see(1e300, -1e300, 0, 0, 0, 0, 0.0, depths.get(), 1.0, 0.0));
        EXPECT(!see(0, 0, 5, 0, 0, 0, 0.0, depths.get(), 1e300, 0.0));      // behind the camera
        EXPECT(!see(0, 0, 4, 0, 0, 0, 0.0, depths.get(), 1e300, 0.0));      // at the centre
        for (double bad : {nan, inf, -inf}) {
            EXPECT(!see(bad, 0, 0, 0, 0, 0, 0.0, depths.get(), 1e300, 0.0));
            EXPECT(!see(0, bad, 0, 0, 0, 0, 0.0, nullptr, 0.0, 0.0));
            EXPECT(!see(0, 0, bad, 0, 0, 1, 0.0, depths.get(), 1e300, 0.0));
        }
    }

    // ---- short points
    EXPECT(is_short(0, 0, 3, 1) && is_short(7, 0, 3, 1) && !is_short(7, 1, 3, 1));
    EXPECT(is_short(7, 1, 3, 2) && !is_short(7, 3, 3, 2) && is_short(5, 3, 3, 2));
    EXPECT(is_short(0xFF, 0xF8, 3, 1));                             // chosen bits at V and above: none
    EXPECT(!is_short(0x8000000000000000ULL, 0x8000000000000000ULL, 64, 1));
    EXPECT(is_short(0x8000000000000000ULL, 0x8000000000000000ULL, 63, 1));
    EXPECT(!is_short(~0ULL, ~0ULL, 64, 64) && is_short(~0ULL >> 1, ~0ULL, 64, 64));
    EXPECT(popcount64(0) == 0 && popcount64(~0ULL) == 64 && popcount64(0x8000000000000001ULL) == 2);
    return finish("overlap");
}
