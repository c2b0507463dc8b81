// Stand-alone host program over raynet_amd/csrc/raynet_views_args.h: the per-view step that
// rn_project_colors, the bake of an atlas and rn_tsdf_integrate share -- project, bilerp and
// observe<1..4> in both modes, with and without depth maps and normals -- on a scene this file
// builds: a handful of views of 3 x 4 pixels and points planted where a load could leave the
// arrays (behind the camera, h2 = 0, dd = 0, NaN and infinite coordinates, X exactly W - 1 and one
// fp64 step beyond it, X = 0.5 / 1.5 / 2.5 for the half-to-even lookup, depths 0, negative, NaN and
// infinite).  Every array has exactly the size of its content, so that an index out of range is an
// error under the address sanitizer.  Every result is compared, bit for bit, with a second,
// straight-line implementation in this file that tests first and loads afterwards, through
// bounds-checked vectors.  The header holds no HIP, so all of it runs here without a GPU.
// tests/test_views_cpu.py builds it with -fsanitize=address,undefined -fno-sanitize-recover=all
// and runs it; it exits 0 when every expectation holds and prints the first one that does not.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "raynet_views_args.h"
#include "host_main.h"

using namespace rn_view;

static const double INF = std::numeric_limits<double>::infinity();
static const double NaN = std::numeric_limits<double>::quiet_NaN();

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// ------------------------------------------------------------------------------ the scene
constexpr int V = 6, H = 3, W = 4;
struct Point {
    double x, y, z, nx, ny, nz;
};
struct Scene {
    std::vector<double> cameras;        // [V][15]
    std::vector<float> depths;          // [V][H][W]
    std::vector<Point> points;
    std::vector<float> images(int C) const {
        std::mt19937 rng(7u + (unsigned)C);
        std::uniform_real_distribution<float> u(0.0f, 1.0f);
        std::vector<float> out((size_t)V * H * W * C);
        for (float &o : out) o = u(rng);
        return out;
    }
};

// a camera that sends every point to pixel (X, Y) at h2
static void constant_camera(std::vector<double> &rows, double X, double Y, double h2, double cx,
                            double cy, double cz) {
    const double row[15] = {0, 0, 0, X * h2, 0, 0, 0, Y * h2, 0, 0, 0, h2, cx, cy, cz};
    rows.insert(rows.end(), row, row + 15);
}

static Scene scene() {
    Scene s;
    const double beyond = std::nextafter((double)(W - 1), INF);
    // views 0 and 1 (a tie): from (0, 0, 4) straight down, focal 4: the point (x, y, 0) lands
    // at pixel (x, y), exactly
    const double down[15] = {4, 0, 0, 0, 0, 4, 0, 0, 0, 0, -1, 4, 0, 0, 4};
    s.cameras.insert(s.cameras.end(), down, down + 15);
    s.cameras.insert(s.cameras.end(), down, down + 15);
    constant_camera(s.cameras, W - 1, 1.0, 4.0, 0, 0, 4);       // 2: X = W - 1 for everybody
    constant_camera(s.cameras, beyond, 1.0, 1.0, 0, 0, 4);      // 3: one fp64 step beyond it
    constant_camera(s.cameras, 1.0, 1.0, 0.0, 0, 0, 4);         // 4: h2 = 0 for everybody
    constant_camera(s.cameras, 2.0, 2.0, 1.0, 1, 1, 0);         // 5: its centre is a planted point
    EXPECT(s.cameras.size() == (size_t)V * CAMERA_DOUBLES);
    EXPECT(s.cameras[3 * 15 + 3] / s.cameras[3 * 15 + 11] == beyond && beyond > W - 1);
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    s.depths.assign((size_t)V * H * W, inf);
    for (int v = 0; v < 2; v++) {
        const float rows[H][W] = {{100.0f, 0.0f, -1.0f, nan},       // Y = 0: the special depths
                                  {100.0f, 0.0f, 100.0f, 0.0f},     // Y = 1: half away from even hides
                                  {inf, 4.5f, 100.0f, 100.0f}};     // Y = 2: (1, 2) is one-sided
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) s.depths[map_index(v, y, x, H, W)] = rows[y][x];
    }
    s.depths[map_index(5, 2, 2, H, W)] = 100.0f;
    const Point planted[] = {
        {0, 0, 5, 0, 0, 0},                     //  0 behind the camera
        {1, 0, 4, 0, 0, 0},                     //  1 on the camera plane: h2 = 0
        {0, 0, 4, 0, 0, 0},                     //  2 at the centre of views 0-4: dd = 0
        {1, 1, 0, 0, 0, 0},                     //  3 at the centre of view 5
        {NaN, 0, 0, 0, 0, 0},                   //  4
        {0, INF, 0, 0, 0, 0},                   //  5
        {0, 0, -INF, 0, 0, 0},                  //  6
        {0, 1, 0, 0, 0, 0},                     //  7 X = 0
        {(double)(W - 1), 2, 0, 0, 0, 0},       //  8 X = W - 1
        {beyond, 1, 0, 0, 0, 0},                //  9 one step beyond
        {0.5, 1, 0, 0, 0, 0},                   // 10 half to even: pixel 0
        {1.5, 1, 0, 0, 0, 0},                   // 11 pixel 2
        {2.5, 1, 0, 0, 0, 0},                   // 12 pixel 2
        {1, 0, 0, 0, 0, 0},                     // 13 depth 0
        {2, 0, 0, 0, 0, 0},                     // 14 depth negative
        {3, 0, 0, 0, 0, 0},                     // 15 depth NaN
        {0, 2, 0, 0, 0, 0},                     // 16 depth inf
        {1, 2, 0, 0, 0, 0},                     // 17 depth 4.5 >= |(1, 2, -4)| = 4.58.. - tol
        {0, (double)(H - 1), 0, 0, 0, 2},       // 18 Y = H - 1, facing
        {1.25, 1.75, 0, 0, 0, -1},              // 19 facing away
        {1.25, 1.75, 0, 1, 0, 0},               // 20 oblique to views 0-4
        {0, 0, 0, 1, 0, 0},                     // 21 exactly perpendicular to views 0-4
        {1.25, 1.75, 0, NaN, 0, 1},             // 22 a NaN normal: nn > 0 fails, as without one
        {-1e300, 1e300, 0, 0, 0, 0},            // 23 far outside
        {1e-320, 1, 0, 0, 0, 1e-170},           // 24 a denormal coordinate; nn underflows to 0
    };
    s.points.assign(planted, planted + sizeof planted / sizeof *planted);
    std::mt19937 rng(3);
    std::uniform_real_distribution<double> at(-1.0, 4.0), up(-1.0, 5.0);
    std::normal_distribution<double> normal(0.0, 1.0);
    for (int k = 0; k < 200; k++)
        s.points.push_back(Point{at(rng), at(rng) * 0.75, k % 3 ? 0.0 : up(rng), normal(rng),
                                 normal(rng), normal(rng) + 1.0});
    return s;
}

// ------------------------------------------------------------------------------ the second loop
struct Seen {
    double X = 0, Y = 0, dx = 0, dy = 0, dz = 0, dd = 0;
    bool ok = false;
};
static Seen straight_project(const std::vector<double> &rows, int v, const Point &p, double border) {
    auto m = [&](int k) { return rows.at((size_t)(15 * v + k)); };
    Seen s;
    double h[3];
    for (int r = 0; r < 3; r++)
        h[r] = ((m(4 * r) * p.x + m(4 * r + 1) * p.y) + m(4 * r + 2) * p.z) + m(4 * r + 3);
    s.X = h[0] / h[2];
    s.Y = h[1] / h[2];
    s.dx = m(12) - p.x, s.dy = m(13) - p.y, s.dz = m(14) - p.z;
    s.dd = (s.dx * s.dx + s.dy * s.dy) + s.dz * s.dz;
    if (!(h[2] > 0.0) || std::isinf(h[2]) || !(s.dd > 0.0)) return s;
    if (!(s.X >= border) || !(s.X <= (double)(W - 1) - border)) return s;
    if (!(s.Y >= border) || !(s.Y <= (double)(H - 1) - border)) return s;
    s.ok = true;
    return s;
}

struct Row {
    float color[4] = {0, 0, 0, 0}, weight = 0;
    uint32_t views = 0;
};
// tests first, loads afterwards: a view that does not count loads nothing at all
static Row straight_observe(const Scene &sc, const std::vector<float> &images, int C,
                            bool with_depths, bool with_normals, double tol, double min_cos,
                            double border, int mode, const Point &q) {
    Point p = q;
    if (!with_normals) p.nx = p.ny = p.nz = 0.0;
    const double nn = (p.nx * p.nx + p.ny * p.ny) + p.nz * p.nz;
    double num[4] = {0, 0, 0, 0}, best[4] = {0, 0, 0, 0}, den = 0.0, best_w = -1.0;
    Row out;
    for (int v = 0; v < V; v++) {
        const Seen s = straight_project(sc.cameras, v, p, border);
        if (!s.ok) continue;
        double w = 1.0;
        if (nn > 0.0) {
            const double dot = (p.nx * s.dx + p.ny * s.dy) + p.nz * s.dz, dot2 = dot * dot;
            if (!(dot > 0.0) || !(dot2 > (min_cos * min_cos) * (nn * s.dd))) continue;
            w = dot2 / (nn * s.dd);
        }
        if (with_depths) {
            const long xr = std::lrint(s.X), yr = std::lrint(s.Y);          // (to nearest even)
            const float zf = sc.depths.at(((size_t)v * H + (size_t)yr) * W + (size_t)xr);
            const double lim = (double)zf + tol;
            if (!(zf > 0.0f) || !(s.dd <= lim * lim)) continue;
        }
        const long x0 = (long)std::floor(s.X), y0 = (long)std::floor(s.Y);
        const long x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
        const double fx = s.X - (double)x0, fy = s.Y - (double)y0;
        auto pixel = [&](long y, long x, int c) {
            return (double)images.at((((size_t)v * H + (size_t)y) * W + (size_t)x) * C + c);
        };
        out.views |= 1u << v;
        den = den + w;
        const bool better = w > best_w;
        if (better) best_w = w;
        for (int c = 0; c < C; c++) {
            const double top = pixel(y0, x0, c) + fx * (pixel(y0, x1, c) - pixel(y0, x0, c));
            const double bot = pixel(y1, x0, c) + fx * (pixel(y1, x1, c) - pixel(y1, x0, c));
            const double col = top + fy * (bot - top);
            num[c] = num[c] + w * col;
            if (better) best[c] = col;
        }
    }
    out.weight = (float)den;
    if (out.views)
        for (int c = 0; c < C; c++) out.color[c] = (float)(mode == 0 ? num[c] / den : best[c]);
    return out;
}

// ------------------------------------------------------------------------------ the checks
static void check_indices_and_bilerp() {
    EXPECT(CAMERA_DOUBLES == 15);
    EXPECT(map_index(0, 0, 0, H, W) == 0 && map_index(V - 1, H - 1, W - 1, H, W) == (size_t)V * H * W - 1);
    EXPECT(map_index(1, 0, 0, H, W) == (size_t)H * W && map_index(0, 1, 0, H, W) == (size_t)W);
    EXPECT(image_index(V - 1, H - 1, W - 1, 2, H, W, 3) == (size_t)V * H * W * 3 - 1);
    EXPECT(image_index(0, 0, 1, 0, H, W, 4) == 4 && image_index(0, 0, 0, 3, H, W, 4) == 3);
    EXPECT(map_index(4095, 46340, 46340, 46341, 46341) == 4096ULL * 46341 * 46341 - 1);
    EXPECT(!pixel_in(-1, W) && !pixel_in(W, W) && pixel_in(0, W) && pixel_in(W - 1, W));
    EXPECT(!pixel_in(std::numeric_limits<int>::min(), W) && !pixel_in(std::numeric_limits<int>::max(), W));
    std::mt19937 rng(1);
    std::uniform_real_distribution<double> u(-2.0, 2.0), f(0.0, 1.0);
    for (int k = 0; k < 1000; k++) {
        const double a = u(rng), b = u(rng), c = u(rng), d = u(rng), fx = f(rng), fy = f(rng);
        const double top = a + fx * (b - a), bot = c + fx * (d - c);
        EXPECT(same(bilerp(a, b, c, d, fx, fy), top + fy * (bot - top)));
        EXPECT(same(bilerp(a, b, c, d, 0.0, 0.0), a) && same(bilerp(a, a, a, a, fx, fy), a));
        EXPECT(same(bilerp(a, b, c, d, 0.0, fy), a + fy * (c - a)));
    }
    EXPECT(std::isnan(bilerp(NaN, 0, 0, 0, 0.5, 0.5)) && std::isnan(bilerp(INF, 0, 0, 0, 1.0, 0.0)));
}

static void check_projections(const Scene &s) {
    const auto cameras = exact(s.cameras);
    int counted = 0;
    for (double border : {0.0, 0.5, 1.0}) {
        const double x_max = (double)(W - 1) - border, y_max = (double)(H - 1) - border;
        for (const Point &p : s.points)
            for (int v = 0; v < V; v++) {
                const Projection got =
                    project(cameras.get() + CAMERA_DOUBLES * v, p.x, p.y, p.z, border, x_max, y_max);
                const Seen want = straight_project(s.cameras, v, p, border);
                EXPECT(same(got.X, want.X) && same(got.Y, want.Y) && same(got.dd, want.dd));
                EXPECT(same(got.dx, want.dx) && same(got.dy, want.dy) && same(got.dz, want.dz));
                EXPECT(got.ok == want.ok);
                if (got.ok) {       // what the callers rely on for their conversions to int
                    EXPECT(got.X >= 0.0 && got.X <= W - 1 && got.Y >= 0.0 && got.Y <= H - 1);
                    counted++;
                }
            }
    }
    EXPECT(counted > 300);
    // the planted points, border 0, by hand
    auto sees = [&](int v, int k) {
        const Point &p = s.points[(size_t)k];
        return project(cameras.get() + CAMERA_DOUBLES * v, p.x, p.y, p.z, 0.0, W - 1.0, H - 1.0).ok;
    };
    for (int k : {0, 1, 2, 4, 5, 6, 9, 23}) EXPECT(!sees(0, k));
    for (int k : {3, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18, 24}) EXPECT(sees(0, k) && sees(1, k));
    for (size_t k = 0; k < s.points.size(); k++) {
        EXPECT(!sees(3, (int)k) && !sees(4, (int)k));           // beyond W - 1; h2 = 0
        const bool finite = std::isfinite(s.points[k].x + s.points[k].y + s.points[k].z);
        if (finite && k != 2) EXPECT(sees(2, (int)k));          // exactly W - 1: in view
    }
    EXPECT(!sees(2, 2) && !sees(2, 4) && !sees(5, 3) && sees(5, 2) && sees(5, 7));
}

template <int C>
static void check_observations(const Scene &s, int &seen_rows, int &differing_modes) {
    const std::vector<float> pictures = s.images(C);
    const auto cameras = exact(s.cameras);
    const auto images = exact(pictures);
    const auto depths = exact(s.depths);
    struct Setting { double tol, min_cos, border; };
    const Setting settings[] = {{0.0, 0.0, 0.0}, {0.1, 0.3, 0.0}, {0.05, 0.0, 0.5}, {1.0, 0.9, 1.0}};
    for (const Setting &t : settings)
        for (int with_depths = 0; with_depths < 2; with_depths++)
            for (int with_normals = 0; with_normals < 2; with_normals++)
                for (const Point &p : s.points) {
                    Row rows[2];
                    for (int mode = 0; mode < 2; mode++) {
                        const Views views{V, cameras.get(), H, W, images.get(),
                                          with_depths ? depths.get() : nullptr, t.tol, t.min_cos,
                                          t.border, mode};
                        const Observation<C> got =
                            with_normals ? observe<C>(views, p.x, p.y, p.z, p.nx, p.ny, p.nz)
                                         : observe<C>(views, p.x, p.y, p.z, 0.0, 0.0, 0.0);
                        const Row want = straight_observe(s, pictures, C, with_depths, with_normals,
                                                          t.tol, t.min_cos, t.border, mode, p);
                        EXPECT(got.views == want.views && same(got.weight, want.weight));
                        for (int c = 0; c < C; c++) EXPECT(same(got.color[c], want.color[c]));
                        if (!got.views) {
                            EXPECT(same(got.weight, 0.0f));
                            for (int c = 0; c < C; c++) EXPECT(same(got.color[c], 0.0f));   // +0
                        }
                        rows[mode] = want;
                        seen_rows += got.views != 0;
                    }
                    EXPECT(rows[0].views == rows[1].views && same(rows[0].weight, rows[1].weight));
                    differing_modes += std::memcmp(rows[0].color, rows[1].color, sizeof rows[0].color) != 0;
                }
    // no view at all: nothing is read, everything is +0
    const Views none{0, nullptr, H, W, nullptr, nullptr, 0.0, 0.0, 0.0, 0};
    const Observation<C> o = observe<C>(none, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0);
    EXPECT(o.views == 0 && same(o.weight, 0.0f) && same(o.color[C - 1], 0.0f));
}

// the planted points by hand: tol = min_cos = border = 0, three channels, with depths and normals
static void check_planted(const Scene &s) {
    const std::vector<float> pictures = s.images(3);
    const auto cameras = exact(s.cameras);
    const auto images = exact(pictures);
    const auto depths = exact(s.depths);
    const Views best{V, cameras.get(), H, W, images.get(), depths.get(), 0.0, 0.0, 0.0, 1};
    auto at = [&](int k) {
        const Point &p = s.points[(size_t)k];
        return observe<3>(best, p.x, p.y, p.z, p.nx, p.ny, p.nz);
    };
    auto pixel = [&](int v, int y, int x, int c) { return pictures[image_index(v, y, x, c, H, W, 3)]; };
    for (int k : {4, 5, 6}) EXPECT(at(k).views == 0 && same(at(k).weight, 0.0f));
    for (int k : {10, 11, 12}) EXPECT((at(k).views & 3u) == 3u);        // half to even: not hidden
    for (int k : {13, 14, 15}) EXPECT((at(k).views & 3u) == 0u);        // depth 0, negative, NaN
    EXPECT((at(16).views & 3u) == 3u);                                  // depth inf hides nothing
    EXPECT((at(17).views & 3u) == 0u);                                  // 4.5^2 < 1 + 4 + 16
    EXPECT((at(19).views & 31u) == 0u && (at(21).views & 31u) == 0u);   // away; perpendicular
    {                                                                   // a NaN normal is none
        const Point &p = s.points[22];
        const Observation<3> bare = observe<3>(best, p.x, p.y, p.z, 0.0, 0.0, 0.0);
        EXPECT(at(22).views == bare.views && bare.views != 0 && same(at(22).weight, bare.weight));
    }
    // exactly on a pixel: the pixel itself, from view 0, the first of the two equal views
    const Observation<3> o = at(7), e = at(8), f = at(18);
    for (int c = 0; c < 3; c++) {
        EXPECT(same(o.color[c], pixel(0, 1, 0, c)) && same(e.color[c], pixel(0, H - 1, W - 1, c)));
        EXPECT(same(f.color[c], pixel(0, H - 1, 0, c)));
    }
    EXPECT((o.views & 7u) == 7u && same(o.weight, 4.0f));               // views 0, 1, 2 and 5
    EXPECT((at(9).views & 3u) == 0u && (at(9).views & 4u) == 4u);
    EXPECT(same(at(24).weight, at(7).weight));                          // nn == 0: weight 1 a view
}

int main() {
    const Scene s = scene();
    check_indices_and_bilerp();
    check_projections(s);
    int seen_rows = 0, differing_modes = 0;
    check_observations<1>(s, seen_rows, differing_modes);
    check_observations<2>(s, seen_rows, differing_modes);
    check_observations<3>(s, seen_rows, differing_modes);
    check_observations<4>(s, seen_rows, differing_modes);
    EXPECT(seen_rows > 2000 && differing_modes > 200);          // (the runs did something)
    check_planted(s);
    return finish("views");
}
