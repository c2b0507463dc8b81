// Stand-alone host program over raynet_amd/csrc/raynet_appearance_args.h: the refusals of
// rn_vertex_area_normals / rn_project_colors, their overflow bounds and accepted edges, and the
// guards and index arithmetic the two kernels read with, which hold no HIP and so run here without
// a GPU.  tests/test_appearance_cpu.py builds it with -fsanitize=address,undefined and runs it; it
// exits 0 when every expectation holds and prints the first one that does not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_appearance_args.h"
#include "host_main.h"

using namespace rn_app;

// what an entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

int main() {
    unsigned char buffer[16] = {0};
    const void *p = buffer;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double inf = std::numeric_limits<double>::infinity();
    const int64_t two31 = (int64_t)1 << 31;

    // ---- rn_vertex_area_normals
    EXPECT(normals_args(true, 756, p, 1508, p, p, p, p) == LAUNCH);
    EXPECT(normals_args(true, 5, p, 0, nullptr, p, nullptr, p) == LAUNCH);   // no faces: zeros
    EXPECT(normals_args(true, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == EMPTY);
    EXPECT(normals_args(true, 0, nullptr, 7, nullptr, nullptr, nullptr, nullptr) == EMPTY);
    EXPECT(status(normals_args(false, 756, p, 1508, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, -1, p, 1508, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 756, p, -1, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 0, p, -1, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 756, nullptr, 1508, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 756, p, 1508, nullptr, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 756, p, 1508, p, nullptr, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 756, p, 1508, p, p, nullptr, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 756, p, 1508, p, p, p, nullptr)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 5, p, 0, nullptr, nullptr, nullptr, p)) == RN_ERR_INVALID);
    // 3 nf and nv + 1 are int32s: in 64-bit arithmetic, no product that could overflow
    EXPECT(normals_args(true, 4, p, 715827882, p, p, p, p) == LAUNCH);      // 3 nf = 2^31 - 2
    EXPECT(3 * (int64_t)715827882 == two31 - 2);
    EXPECT(status(normals_args(true, 4, p, 715827883, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, 4, p, std::numeric_limits<int64_t>::max(), p, p, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(normals_args(true, two31 - 2, p, 4, p, p, p, p) == LAUNCH);
    EXPECT(status(normals_args(true, two31 - 1, p, 4, p, p, p, p)) == RN_ERR_INVALID);
    EXPECT(status(normals_args(true, std::numeric_limits<int64_t>::max(), p, 4, p, p, p, p)) ==
           RN_ERR_INVALID);

    // ---- rn_project_colors
    auto colors = [&](int64_t n, int32_t V, int32_t H, int32_t W, int32_t C, double tol,
                      double min_cos, double border, int32_t mode) {
        return colors_args(true, n, p, V, p, H, W, C, p, tol, min_cos, border, mode, p, p, p);
    };
    EXPECT(colors(300, 5, 24, 32, 3, 0.1, 0.2, 1.5, 0) == LAUNCH);
    EXPECT(colors(300, 5, 24, 32, 3, 0.1, 0.2, 1.5, 1) == LAUNCH);
    EXPECT(colors(1, 32, 1, 1, 4, 0.0, 0.0, 0.0, 0) == LAUNCH);             // the accepted edges
    EXPECT(colors(1, 0, 1, 1, 1, 0.0, 0.0, 0.0, 0) == LAUNCH);              // V == 0: rows of zeros
    EXPECT(colors(1, 1, 1, 1, 1, 0.0, std::nextafter(1.0, 0.0), 1e300, 1) == LAUNCH);
    EXPECT(colors(0, 5, 24, 32, 3, 0.1, 0.2, 1.5, 0) == EMPTY);
    EXPECT(colors_args(true, 0, nullptr, 5, nullptr, 24, 32, 3, nullptr, 0.0, 0.0, 0.0, 0,
                       nullptr, nullptr, nullptr) == EMPTY);
    EXPECT(colors_args(true, 3, p, 0, nullptr, 24, 32, 3, nullptr, 0.0, 0.0, 0.0, 0, p, p, p) ==
           LAUNCH);
    EXPECT(status(colors(-1, 5, 24, 32, 3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, -1, 24, 32, 3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 33, 24, 32, 3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 0, 32, 3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 0, 3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, -24, 32, 3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 0, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 5, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, -3, 0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, -0.1, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, nan, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, inf, 0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, -0.2, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, 1.0, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, nan, 1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, 0.2, -1.5, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, 0.2, nan, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, 0.2, inf, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, 0.2, 1.5, 2)) == RN_ERR_INVALID);
    EXPECT(status(colors(300, 5, 24, 32, 3, 0.1, 0.2, 1.5, -1)) == RN_ERR_INVALID);
    EXPECT(status(colors_args(false, 300, p, 5, p, 24, 32, 3, p, 0.1, 0.2, 1.5, 0, p, p, p)) ==
           RN_ERR_INVALID);
    // every required pointer on its own
    EXPECT(status(colors_args(true, 300, nullptr, 5, p, 24, 32, 3, p, 0.1, 0.2, 1.5, 0, p, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(colors_args(true, 300, p, 5, nullptr, 24, 32, 3, p, 0.1, 0.2, 1.5, 0, p, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(colors_args(true, 300, p, 5, p, 24, 32, 3, nullptr, 0.1, 0.2, 1.5, 0, p, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(colors_args(true, 300, p, 5, p, 24, 32, 3, p, 0.1, 0.2, 1.5, 0, nullptr, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(colors_args(true, 300, p, 5, p, 24, 32, 3, p, 0.1, 0.2, 1.5, 0, p, nullptr, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(colors_args(true, 300, p, 5, p, 24, 32, 3, p, 0.1, 0.2, 1.5, 0, p, p, nullptr)) ==
           RN_ERR_INVALID);
    // n C is an int32
    EXPECT(colors(two31 - 1, 1, 8, 8, 1, 0.0, 0.0, 0.0, 0) == LAUNCH);
    EXPECT(status(colors(two31, 1, 8, 8, 1, 0.0, 0.0, 0.0, 0)) == RN_ERR_INVALID);
    EXPECT(colors(715827882, 1, 8, 8, 3, 0.0, 0.0, 0.0, 0) == LAUNCH);
    EXPECT(status(colors(715827883, 1, 8, 8, 3, 0.0, 0.0, 0.0, 0)) == RN_ERR_INVALID);
    EXPECT(colors(536870911, 1, 8, 8, 4, 0.0, 0.0, 0.0, 0) == LAUNCH);
    EXPECT(status(colors(536870912, 1, 8, 8, 4, 0.0, 0.0, 0.0, 0)) == RN_ERR_INVALID);
    EXPECT(status(colors(std::numeric_limits<int64_t>::max(), 1, 8, 8, 4, 0.0, 0.0, 0.0, 0)) ==
           RN_ERR_INVALID);

    // ---- the normals kernel's reads: heap arrays of exactly the stated sizes take every guarded
    // read (the address sanitizer watches the ends) whatever the index arrays hold
    const int64_t nv = 5, nf = 4;
    std::vector<float> vertices(3 * nv, 1.0f);
    std::vector<int32_t> faces = {0, 1, 2, 0, 3, 1, 0, 2, 3, 1, 3, 77};             // one bad index
    std::vector<int32_t> corners = {0, 3, 6, -4, 12, 99, 2, 5, 8, 7, 10, 1 << 30};  // bad corners
    std::vector<int32_t> offsets = {-9, 3, 6, 9, 1 << 30, -1};                      // bad offsets
    EXPECT((int64_t)faces.size() == 3 * nf && (int64_t)corners.size() == 3 * nf &&
           (int64_t)offsets.size() == nv + 1);
    double touched = 0.0;
    int64_t visited = 0;
    for (int64_t v = -2; v < nv + 2; v++) {
        if (!vertex_in(v, nv)) continue;
        const int64_t first = clamp_slot(offsets[(size_t)v], nf),
                      last = clamp_slot(offsets[(size_t)v + 1], nf);
        EXPECT(first >= 0 && last <= 3 * nf);
        for (int64_t k = first; k < last; k++) {
            EXPECT(k >= 0 && k < (int64_t)corners.size());
            const int64_t c = corners[(size_t)k];
            if (!corner_in(c, nf)) continue;
            const int64_t f = c / 3;
            bool ok = true;
            for (int s = 0; s < 3; s++) ok = ok && vertex_in(faces[xyz_index(f, s)], nv);
            if (!ok) continue;
            for (int s = 0; s < 3; s++)
                for (int a = 0; a < 3; a++)
                    touched += vertices[xyz_index(faces[xyz_index(f, s)], a)];
            visited++;
        }
    }
    EXPECT(visited == 3 + 0 + 3 + 1 && touched == 9.0 * (double)visited);
    EXPECT(!corner_in(-1, nf) && !corner_in(12, nf) && corner_in(11, nf) && corner_in(0, nf));
    EXPECT(!vertex_in(-1, nv) && !vertex_in(5, nv) && vertex_in(4, nv) && !vertex_in(0, 0));
    EXPECT(clamp_slot(-5, nf) == 0 && clamp_slot(13, nf) == 12 && clamp_slot(7, nf) == 7 &&
           clamp_slot(7, 0) == 0);
    EXPECT(xyz_index(0x7ffffffeLL, 2) == 3 * (size_t)0x7ffffffeULL + 2);    // no 32-bit overflow

    // ---- the colour kernel's reads: the last pixel of the last view, and pixel 0 for the rest
    const int V = 3, H = 5, W = 7, C = 4;
    std::vector<float> images((size_t)V * H * W * C, 0.5f), depths((size_t)V * H * W, 2.0f);
    EXPECT(image_index(V - 1, H - 1, W - 1, C - 1, H, W, C) == images.size() - 1);
    EXPECT(depth_index(V - 1, H - 1, W - 1, H, W) == depths.size() - 1);
    EXPECT(image_index(0, 0, 0, 0, H, W, C) == 0 && depth_index(0, 0, 0, H, W) == 0);
    double sum = 0.0;
    for (int v = 0; v < V; v++)
        for (int y = -2; y < H + 2; y++)
            for (int x = -2; x < W + 2; x++) {
                const int ys = pixel_in(y, H) ? y : 0, xs = pixel_in(x, W) ? x : 0;
                sum += depths[depth_index(v, ys, xs, H, W)];
                for (int c = 0; c < C; c++) sum += images[image_index(v, ys, xs, c, H, W, C)];
            }
    EXPECT(sum == 4.0 * V * (H + 4) * (W + 4));
    // 32 views of 16384 x 16384 x 4: beyond 32 bits, within size_t
    EXPECT(image_index(31, 16383, 16383, 3, 16384, 16384, 4) == 32ULL * 16384 * 16384 * 4 - 1);
    EXPECT(MAX_VIEWS == 32 && MAX_CHANNELS == 4 && CAMERA_DOUBLES == 15);
    return finish("appearance");
}
