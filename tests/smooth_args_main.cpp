// Stand-alone host program over raynet_amd/csrc/raynet_smooth_args.h: the refusals of
// rn_mesh_smooth at every limit and one beyond it, the workspace layout and the ping-pong parity,
// and whole smoothings of small meshes -- the ring entries and the steps of all vertices by the
// header's functions, launch by launch as the entry makes them -- inside exactly-sized heap
// buffers, so that an access out of bounds is an error under the address sanitizer.  The meshes
// carry planted out-of-range corners and face indices and reversed and overhanging `offsets`
// ranges.  Every result is compared, bit for bit, with a second, straightforward loop in this file
// that walks corners -> faces -> vertices without a ring.  The header holds no HIP, so all of it
// runs here without a GPU.  tests/test_smooth_cpu.py builds it with
// -fsanitize=address,undefined -fno-sanitize-recover=all and runs it; it exits 0 when every
// expectation holds and prints the first one that does not.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_smooth_args.h"
#include "host_main.h"

using namespace rn_sm;

static const double INF = std::numeric_limits<double>::infinity();
static const double NaN = std::numeric_limits<double>::quiet_NaN();

// what the entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

// ------------------------------------------------------------------------------ the verdict
struct Call {
    bool ctx = true;
    int64_t nv = 10, nf = 4;
    const void *in, *faces, *offsets, *corners, *workspace, *out;
    int32_t iterations = 10;
    double lambda = 0.5, mu = -0.53, max_move = INF;
    Verdict verdict() const {
        return smooth_args(ctx, nv, in, nf, faces, offsets, corners, iterations, lambda, mu,
                           max_move, workspace, out);
    }
};

static void check_verdicts() {
    alignas(8) static char a[64], b[64], c[64], d[64], e[64], w[64];
    Call good;
    good.in = a, good.faces = b, good.offsets = c, good.corners = d, good.out = e, good.workspace = w;
    EXPECT(good.verdict() == LAUNCH);
    Call x = good;
#define REFUSED(change)                              \
    x = good;                                        \
    change;                                          \
    EXPECT(status(x.verdict()) == RN_ERR_INVALID)
#define TAKEN(change, what)                          \
    x = good;                                        \
    change;                                          \
    EXPECT(x.verdict() == what)
    REFUSED(x.ctx = false);
    // the sizes: the limit and one beyond
    REFUSED(x.nv = -1);
    REFUSED(x.nf = -1);
    TAKEN(x.nv = INT32_LIMIT - 1, LAUNCH);
    REFUSED(x.nv = INT32_LIMIT);
    REFUSED(x.nv = (int64_t)1 << 40);
    TAKEN(x.nf = INT32_LIMIT / 3, LAUNCH);                  // 3 nf == 2^31 - 1 - 1
    REFUSED(x.nf = INT32_LIMIT / 3 + 1);
    REFUSED(x.nf = (int64_t)1 << 40);
    EXPECT(3 * (INT32_LIMIT / 3) <= INT32_LIMIT && 3 * (INT32_LIMIT / 3 + 1) > INT32_LIMIT);
    // the iterations
    REFUSED(x.iterations = -1);
    TAKEN(x.iterations = 0, LAUNCH);
    TAKEN(x.iterations = MAX_ITERATIONS, LAUNCH);
    REFUSED(x.iterations = MAX_ITERATIONS + 1);
    REFUSED(x.iterations = std::numeric_limits<int32_t>::min());
    // lambda in (0, 1]
    REFUSED(x.lambda = 0.0);
    REFUSED(x.lambda = -0.5);
    TAKEN(x.lambda = std::numeric_limits<double>::denorm_min(), LAUNCH);
    TAKEN(x.lambda = 1.0, LAUNCH);
    REFUSED(x.lambda = std::nextafter(1.0, 2.0));
    REFUSED(x.lambda = INF);
    REFUSED(x.lambda = NaN);
    // mu in [-1, 0]
    TAKEN(x.mu = 0.0, LAUNCH);
    TAKEN(x.mu = -0.0, LAUNCH);
    TAKEN(x.mu = -1.0, LAUNCH);
    REFUSED(x.mu = std::nextafter(-1.0, -2.0));
    REFUSED(x.mu = std::numeric_limits<double>::denorm_min());
    REFUSED(x.mu = -INF);
    REFUSED(x.mu = NaN);
    // max_move > 0, +inf included
    REFUSED(x.max_move = 0.0);
    REFUSED(x.max_move = -1.0);
    REFUSED(x.max_move = -INF);
    REFUSED(x.max_move = NaN);
    TAKEN(x.max_move = std::numeric_limits<double>::denorm_min(), LAUNCH);
    TAKEN(x.max_move = INF, LAUNCH);
    // the pointers
    REFUSED(x.in = nullptr);
    REFUSED(x.offsets = nullptr);
    REFUSED(x.out = nullptr);
    REFUSED(x.workspace = nullptr);
    REFUSED(x.faces = nullptr);
    REFUSED(x.corners = nullptr);
    TAKEN((x.nf = 0, x.faces = nullptr, x.corners = nullptr), LAUNCH);
    REFUSED(x.workspace = w + 4);
    REFUSED(x.workspace = w + 1);
    TAKEN(x.workspace = w + 8, LAUNCH);
    REFUSED(x.out = x.in);
    REFUSED(x.out = x.workspace);
    REFUSED(x.in = x.workspace);
    // nothing to write: EMPTY whatever the pointers, but the scalars are looked at first
    TAKEN((x.nv = 0, x.in = x.out = x.workspace = x.offsets = nullptr), EMPTY);
    REFUSED((x.nv = 0, x.iterations = -1));
    REFUSED((x.nv = 0, x.lambda = 2.0));
    EXPECT(status(EMPTY) == RN_OK && status(LAUNCH) == RN_OK);
#undef REFUSED
#undef TAKEN
}

static void check_layout_and_parity() {
    EXPECT(workspace_bytes(0, 0) == 0 && workspace_bytes(1, 0) == 16 && workspace_bytes(2, 0) == 24);
    EXPECT(workspace_bytes(3, 1) == 24 + 40 && scratch_offset(1) == 24 && scratch_offset(7) % 8 == 0);
    EXPECT(workspace_bytes(INT32_LIMIT - 1, INT32_LIMIT / 3) > 0);
    EXPECT(sizes_ok(0, 0) && !sizes_ok(-1, 0) && !sizes_ok(0, -1) && !sizes_ok(INT32_LIMIT, 0));
    EXPECT(blocks(0, 256) == 1 && blocks(256, 256) == 1 && blocks(257, 256) == 2);
    EXPECT(blocks((int64_t)1 << 40, 256) == MAX_BLOCKS);
    EXPECT(step_count(10, -0.53) == 20 && step_count(10, 0.0) == 10 && step_count(10, -0.0) == 10);
    EXPECT(step_count(0, -0.53) == 0 && step_count(MAX_ITERATIONS, -1.0) == 20000);
    float in[3], scratch[3], out[3];
    for (int64_t L = 1; L <= 7; L++) {
        EXPECT(step_target(L, L, scratch, out) == out);                 // the last step writes out
        EXPECT(step_source(1, L, in, scratch, out) == in);              // the first one reads in
        for (int64_t i = 1; i <= L; i++) {
            const float *src = step_source(i, L, in, scratch, out);
            float *dst = step_target(i, L, scratch, out);
            EXPECT(src != dst && dst != in);
            if (i > 1) EXPECT(src == step_target(i - 1, L, scratch, out));
        }
    }
    for (int64_t i = 1; i <= 6; i++) {
        EXPECT(step_factor(i, 0.5, -0.53) == (i % 2 ? 0.5 : -0.53));
        EXPECT(step_factor(i, 0.5, 0.0) == 0.5);
    }
}

// ------------------------------------------------------------------------------ the meshes
struct Mesh {
    int64_t nv = 0;
    std::vector<float> vertices;            // [nv][3]
    std::vector<int32_t> faces;             // [nf][3]
    std::vector<int32_t> offsets, corners;  // the corner table, garbage included
    std::vector<uint8_t> fixed;             // empty for none
    int64_t nf() const { return (int64_t)faces.size() / 3; }
};

static void positions(Mesh &m, unsigned seed) {
    std::mt19937 rng(seed);
    std::normal_distribution<float> normal(0.0f, 1.0f);
    m.vertices.resize(3 * (size_t)m.nv);
    for (int64_t v = 0; v < m.nv; v++)
        for (int k = 0; k < 3; k++) m.vertices[xyz_index(v, k)] = (k == 0 ? (float)v : 0.0f) + normal(rng);
}

// the corner table of the faces as they are: the corners whose vertex is in range, by vertex
static void corner_table(Mesh &m) {
    std::vector<std::vector<int32_t>> rows((size_t)m.nv);
    for (int64_t c = 0; c < 3 * m.nf(); c++)
        if (vertex_in(m.faces[(size_t)c], m.nv)) rows[(size_t)m.faces[(size_t)c]].push_back((int32_t)c);
    m.offsets.assign(1, 0);
    m.corners.clear();
    for (const auto &row : rows) {
        m.corners.insert(m.corners.end(), row.begin(), row.end());
        m.offsets.push_back((int32_t)m.corners.size());
    }
    m.corners.resize(3 * (size_t)m.nf(), -1);   // (corners of out-of-range indices: named by no row)
}

static Mesh strip(int32_t nv, unsigned seed) {
    Mesh m;
    m.nv = nv;
    for (int32_t i = 0; i + 2 < nv; i++) m.faces.insert(m.faces.end(), {i, i + 1, i + 2});
    positions(m, seed);
    corner_table(m);
    return m;
}

static Mesh star(int32_t nf, bool hub_last, unsigned seed) {
    Mesh m;
    m.nv = 2 * nf + 1;
    for (int32_t i = 0; i < nf; i++) {
        if (hub_last) m.faces.insert(m.faces.end(), {(int32_t)m.nv - 1, 2 * i, 2 * i + 1});
        else m.faces.insert(m.faces.end(), {0, 2 * i + 1, 2 * i + 2});
    }
    positions(m, seed);
    corner_table(m);
    return m;
}

static Mesh tetrahedron(unsigned seed) {
    Mesh m;
    m.nv = 4;
    m.faces = {0, 1, 2, 0, 3, 1, 1, 3, 2, 0, 2, 3};
    positions(m, seed);
    corner_table(m);
    return m;
}

// vertex ids permuted, faces shuffled, the table rebuilt
static Mesh shuffled(const Mesh &in, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<int32_t> order((size_t)in.nv);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<int64_t> rows((size_t)in.nf());
    std::iota(rows.begin(), rows.end(), 0);
    std::shuffle(rows.begin(), rows.end(), rng);
    Mesh m;
    m.nv = in.nv;
    m.vertices.resize(in.vertices.size());
    for (int64_t v = 0; v < in.nv; v++)
        for (int k = 0; k < 3; k++)
            m.vertices[xyz_index(order[(size_t)v], k)] = in.vertices[xyz_index(v, k)];
    for (int64_t r : rows)
        for (int k = 0; k < 3; k++) m.faces.push_back(order[(size_t)in.faces[xyz_index(r, k)]]);
    corner_table(m);
    return m;
}

// garbage planted in all three index arrays, after the table was built
static Mesh planted(Mesh m, unsigned seed) {
    std::mt19937 rng(seed);
    const int32_t bad_vertex[] = {-1, (int32_t)m.nv, std::numeric_limits<int32_t>::max(),
                                  std::numeric_limits<int32_t>::min()};
    const int32_t bad_corner[] = {-1, (int32_t)(3 * m.nf()), std::numeric_limits<int32_t>::max(),
                                  std::numeric_limits<int32_t>::min()};
    for (size_t i = 0; i < m.faces.size(); i++)
        if (rng() % 16 == 0) m.faces[i] = bad_vertex[rng() % 4];
    for (size_t i = 0; i < m.corners.size(); i++)
        if (rng() % 16 == 0) m.corners[i] = bad_corner[rng() % 4];
    // reversed, overhanging and negative ranges
    const int32_t bad_offset[] = {-1, std::numeric_limits<int32_t>::min(), (int32_t)(3 * m.nf() + 1),
                                  std::numeric_limits<int32_t>::max(), 0, (int32_t)(3 * m.nf())};
    for (size_t i = 0; i < m.offsets.size(); i++)
        if (rng() % 8 == 0) m.offsets[i] = bad_offset[rng() % 6];
    return m;
}

// ------------------------------------------------------------------------------ two smoothings
// as rn_mesh_smooth runs it: the header's functions, "launch" by "launch", in exactly-sized buffers
static std::vector<float> by_the_header(const Mesh &m, int32_t iterations, double lambda, double mu,
                                        double max_move) {
    const int64_t nv = m.nv, nf = m.nf();
    const auto in = exact(m.vertices);
    const auto faces = exact(m.faces);
    const auto offsets = exact(m.offsets);
    const auto corners = exact(m.corners);
    const auto fixed = exact(m.fixed);
    const uint8_t *pinned = m.fixed.empty() ? nullptr : fixed.get();
    const int64_t bytes = workspace_bytes(nv, nf);
    char *workspace = (char *)std::malloc((size_t)bytes);           // 16-byte aligned, exact
    std::unique_ptr<float[]> out(new float[3 * (size_t)nv]);
    std::memset(workspace, 0xa5, (size_t)bytes);
    EXPECT(smooth_args(true, nv, in.get(), nf, faces.get(), offsets.get(), corners.get(), iterations,
                       lambda, mu, max_move, workspace, out.get()) == LAUNCH);
    int32_t *ring = (int32_t *)workspace;
    float *scratch = (float *)(workspace + scratch_offset(nf));
    const int64_t L = step_count(iterations, mu);
    if (L == 0) std::copy(in.get(), in.get() + 3 * nv, out.get());
    else {
        for (int64_t k = 0; corner_in(k, nf); k++) ring_entry(k, nv, nf, faces.get(), corners.get(), ring);
        for (int64_t i = 1; i <= L; i++) {
            const float *src = step_source(i, L, in.get(), scratch, out.get());
            float *dst = step_target(i, L, scratch, out.get());
            for (int64_t v = 0; vertex_in(v, nv); v++)
                step_vertex(v, nv, nf, offsets.get(), ring, pinned, in.get(), src,
                            step_factor(i, lambda, mu), max_move, dst);
        }
    }
    // vertices_in is never written
    EXPECT(std::memcmp(in.get(), m.vertices.data(), 12 * (size_t)nv) == 0);
    std::vector<float> result(out.get(), out.get() + 3 * nv);
    std::free(workspace);
    return result;
}

// the second loop: straightforward, corners -> faces -> vertices, two vectors swapped
static std::vector<float> straightforward(const Mesh &m, int32_t iterations, double lambda,
                                          double mu, double max_move) {
    const int64_t nv = m.nv, nf = m.nf();
    std::vector<float> now = m.vertices, next(m.vertices.size());
    auto one = [&](double t) {
        for (int64_t v = 0; v < nv; v++) {
            double s[3] = {0.0, 0.0, 0.0};
            int64_t count = 0;
            int64_t first = m.offsets[(size_t)v], last = m.offsets[(size_t)v + 1];
            first = std::min(std::max(first, (int64_t)0), 3 * nf);
            last = std::min(std::max(last, (int64_t)0), 3 * nf);
            for (int64_t k = first; k < last; k++) {
                const int64_t c = m.corners.at((size_t)k);
                if (c < 0 || c >= 3 * nf) continue;
                const int64_t f = c / 3, slot = c % 3;
                bool inside = true;
                for (int j = 0; j < 3; j++) {
                    const int64_t i = m.faces.at((size_t)(3 * f + j));
                    inside = inside && i >= 0 && i < nv;
                }
                if (!inside) continue;
                const int64_t a = m.faces.at((size_t)(3 * f + (slot + 1) % 3)),
                              b = m.faces.at((size_t)(3 * f + (slot + 2) % 3));
                for (int j = 0; j < 3; j++)
                    s[j] = (s[j] + (double)now.at((size_t)(3 * a + j))) + (double)now.at((size_t)(3 * b + j));
                count += 2;
            }
            for (int j = 0; j < 3; j++) {
                const size_t at = (size_t)(3 * v + j);
                if (count == 0 || (!m.fixed.empty() && m.fixed[(size_t)v])) {
                    next[at] = now[at];
                    continue;
                }
                const double p = (double)now[at];
                double x = p + t * (s[j] / (double)count - p);
                const double lo = (double)m.vertices[at] - max_move, hi = (double)m.vertices[at] + max_move;
                if (x < lo) x = lo;
                if (x > hi) x = hi;
                next[at] = (float)x;
            }
        }
        now.swap(next);
    };
    for (int32_t i = 0; i < iterations; i++) {
        one(lambda);
        if (mu != 0.0) one(mu);
    }
    return now;
}

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), 4 * a.size()) == 0);
}

static void check_smoothings() {
    std::vector<Mesh> meshes;
    Mesh none;
    none.nv = 5;
    positions(none, 1);
    corner_table(none);
    meshes.push_back(none);                                 // vertices and no face
    Mesh one = strip(3, 2);
    meshes.push_back(one);
    meshes.push_back(tetrahedron(3));
    for (int32_t nv : {4, 64, 65, 257}) {
        meshes.push_back(strip(nv, (unsigned)nv));
        meshes.push_back(shuffled(strip(nv, (unsigned)nv), (unsigned)nv + 1));
    }
    meshes.push_back(star(50, false, 5));
    meshes.push_back(star(50, true, 6));
    const size_t clean = meshes.size();
    for (size_t i = 0; i < clean; i++)
        for (unsigned seed : {11u, 12u, 13u}) meshes.push_back(planted(meshes[i], seed + (unsigned)i));
    // pins, and non-finite positions
    Mesh pinned = shuffled(strip(65, 7), 8);
    pinned.fixed.assign((size_t)pinned.nv, 0);
    for (size_t v = 0; v < pinned.fixed.size(); v += 5) pinned.fixed[v] = (uint8_t)(1 + v);
    meshes.push_back(pinned);
    meshes.push_back(planted(pinned, 21));
    Mesh poisoned = strip(64, 9);
    poisoned.vertices[xyz_index(20, 1)] = std::numeric_limits<float>::quiet_NaN();
    poisoned.vertices[xyz_index(40, 2)] = std::numeric_limits<float>::infinity();
    meshes.push_back(poisoned);

    struct Run { int32_t iterations; double lambda, mu, max_move; };
    const Run runs[] = {{0, 0.5, -0.53, INF}, {1, 0.5, -0.53, INF}, {2, 0.5, -0.53, INF},
                        {3, 0.5, -0.53, 0.05}, {1, 0.5, 0.0, INF}, {2, 1.0, -1.0, 0.25},
                        {10, 0.5, -0.53, 1.0}};
    int moved = 0;
    for (const Mesh &m : meshes)
        for (const Run &r : runs) {
            const std::vector<float> a = by_the_header(m, r.iterations, r.lambda, r.mu, r.max_move);
            const std::vector<float> b = straightforward(m, r.iterations, r.lambda, r.mu, r.max_move);
            EXPECT(same_bits(a, b));
            if (r.iterations == 0) EXPECT(same_bits(a, m.vertices));
            if (!same_bits(a, m.vertices)) moved++;
            // the clamp, and the pins
            for (size_t i = 0; i < a.size(); i++) {
                const double lo = (double)m.vertices[i] - r.max_move, hi = (double)m.vertices[i] + r.max_move;
                if (std::isfinite(a[i]) && std::isfinite(m.vertices[i]))
                    EXPECT(a[i] >= (float)lo && a[i] <= (float)hi);
                if (!m.fixed.empty() && m.fixed[i / 3])
                    EXPECT(std::memcmp(&a[i], &m.vertices[i], 4) == 0);
            }
        }
    EXPECT(moved > 100);                                    // (the runs did something)
    // the NaN of `poisoned` after one step: vertex 20 and its face neighbours 18 .. 22, in y only
    const std::vector<float> p = by_the_header(poisoned, 1, 0.5, 0.0, INF);
    for (int64_t v = 0; v < poisoned.nv; v++) {
        EXPECT(std::isnan(p[xyz_index(v, 1)]) == (v >= 18 && v <= 22));
        EXPECT(std::isfinite(p[xyz_index(v, 0)]));
        EXPECT(std::isfinite(p[xyz_index(v, 2)]) == !(v >= 38 && v <= 42));
    }
}

int main() {
    check_verdicts();
    check_layout_and_parity();
    check_smoothings();
    return finish("smooth");
}
