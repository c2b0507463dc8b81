// Stand-alone host program over raynet_amd/csrc/raynet_components_args.h: the refusals of
// rn_mesh_components and its accepted edges, which faces count, the launch geometry, and the
// union-find itself -- unite / find with the __atomic builtins on plain int32_t, run by 8 threads
// over the faces of strips, stars and shuffled meshes and compared with a sequential union-find.
// The header holds no HIP, so all of it runs here without a GPU.  tests/test_components_cpu.py
// builds it twice -- with -fsanitize=address,undefined and with -fsanitize=thread -- and runs it;
// it exits 0 when every expectation holds and prints the first one that does not.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_components_args.h"
#include "host_main.h"

using namespace rn_cc;

// what the entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

// the atomics policy on the host: relaxed, on plain int32_t
struct HostAtomics {
    int32_t *parent;
    int32_t load(int32_t x) const { return __atomic_load_n(parent + x, __ATOMIC_RELAXED); }
    int32_t cas(int32_t x, int32_t expect, int32_t value) const {
        __atomic_compare_exchange_n(parent + x, &expect, value, false, __ATOMIC_RELAXED,
                                    __ATOMIC_RELAXED);
        return expect;
    }
    void store(int32_t x, int32_t value) const { __atomic_store_n(parent + x, value, __ATOMIC_RELAXED); }
};

struct Mesh {
    int32_t nv;
    std::vector<int32_t> faces;             // [nf][3]
    int64_t nf() const { return (int64_t)faces.size() / 3; }
};

static Mesh strip(int32_t nv) {
    Mesh m{nv, {}};
    for (int32_t i = 0; i + 2 < nv; i++) m.faces.insert(m.faces.end(), {i, i + 1, i + 2});
    return m;
}

static Mesh star(int32_t nf, bool hub_last) {
    Mesh m{2 * nf + 1, {}};
    for (int32_t i = 0; i < nf; i++) {
        if (hub_last) m.faces.insert(m.faces.end(), {m.nv - 1, 2 * i, 2 * i + 1});
        else m.faces.insert(m.faces.end(), {0, 2 * i + 1, 2 * i + 2});
    }
    return m;
}

// disjoint triangles and tetrahedra, some vertices in no face, some faces out of range
static Mesh pieces(int32_t n) {
    Mesh m{7 * n + 5, {}};
    for (int32_t i = 0; i < n; i++) {
        const int32_t t = 7 * i, q = 7 * i + 3;
        m.faces.insert(m.faces.end(), {t, t + 1, t + 2});
        m.faces.insert(m.faces.end(), {q, q + 1, q + 2, q, q + 3, q + 1, q + 1, q + 3, q + 2, q, q + 2, q + 3});
        if (i % 9 == 0) m.faces.insert(m.faces.end(), {t, -1, q});
        if (i % 11 == 0) m.faces.insert(m.faces.end(), {t, q, m.nv});
        if (i % 13 == 0) m.faces.insert(m.faces.end(), {q, q, q});
        if (i % 17 == 0 && i) m.faces.insert(m.faces.end(), {t, t, t - 7});     // (a, a, b)
    }
    return m;
}

// vertex ids permuted, faces shuffled
static Mesh shuffled(const Mesh &in, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<int32_t> order((size_t)in.nv);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);
    std::vector<int64_t> rows((size_t)in.nf());
    std::iota(rows.begin(), rows.end(), 0);
    std::shuffle(rows.begin(), rows.end(), rng);
    Mesh m{in.nv, {}};
    for (int64_t r : rows)
        for (int k = 0; k < 3; k++) {
            const int32_t v = in.faces[face_index(r, k)];
            m.faces.push_back(vertex_in(v, in.nv) ? order[(size_t)v] : v);
        }
    return m;
}

static std::vector<int32_t> sequential(const Mesh &m) {
    std::vector<int32_t> parent((size_t)m.nv);
    std::iota(parent.begin(), parent.end(), 0);
    auto root = [&](int32_t x) {
        while (parent[(size_t)x] != x) x = parent[(size_t)x];
        return x;
    };
    auto join = [&](int32_t a, int32_t b) {
        a = root(a);
        b = root(b);
        if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
    };
    for (int64_t f = 0; f < m.nf(); f++) {
        const int32_t a = m.faces[face_index(f, 0)], b = m.faces[face_index(f, 1)],
                      c = m.faces[face_index(f, 2)];
        if (!face_counts_in(m.nv, a, b, c)) continue;
        join(a, b);
        join(b, c);
    }
    std::vector<int32_t> labels((size_t)m.nv);
    for (int32_t v = 0; v < m.nv; v++) labels[(size_t)v] = root(v);
    return labels;
}

// the kernels' work on `threads` host threads: init, hook (the faces dealt out round robin, as a
// grid-stride loop deals them), flatten
static std::vector<int32_t> concurrent(const Mesh &m, int threads, bool *ok) {
    std::vector<int32_t> parent((size_t)m.nv);
    std::iota(parent.begin(), parent.end(), 0);
    const HostAtomics at{parent.data()};
    const int64_t bound = step_bound(m.nv);
    std::vector<int> good((size_t)threads, 1);
    auto hook = [&](int t) {
        for (int64_t f = t; f < m.nf(); f += threads) {
            const int32_t a = m.faces[face_index(f, 0)], b = m.faces[face_index(f, 1)],
                          c = m.faces[face_index(f, 2)];
            if (!face_counts_in(m.nv, a, b, c)) continue;
            if (!unite(at, a, b, bound) || !unite(at, b, c, bound)) good[(size_t)t] = 0;
        }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(hook, t);
    for (auto &th : pool) th.join();
    pool.clear();
    // the invariant, and flatten in a later "launch"
    for (int32_t v = 0; v < m.nv; v++) EXPECT(parent[(size_t)v] <= v);
    // (k_cc_flatten's own code: the chase by loads and one store per vertex, racing with the
    // other threads' chases through the same words)
    auto flatten = [&](int t) {
        for (int32_t v = t; v < m.nv; v += threads)
            if (!rn_cc::flatten(at, v, bound)) good[(size_t)t] = 0;
    };
    for (int t = 0; t < threads; t++) pool.emplace_back(flatten, t);
    for (auto &th : pool) th.join();
    *ok = std::all_of(good.begin(), good.end(), [](int g) { return g == 1; });
    return parent;
}

static void check(const Mesh &m, const char *what) {
    bool ok = false;
    const std::vector<int32_t> got = concurrent(m, 8, &ok), want = sequential(m);
    if (!ok || got != want) {
        std::printf("%s: nv %d nf %lld: %s\n", what, (int)m.nv, (long long)m.nf(),
                    ok ? "labels differ from the sequential union-find" : "a bound was reached");
        failures++;
    }
    for (int32_t v = 0; v < m.nv; v++) {
        const int32_t r = got[(size_t)v];
        if (!(r >= 0 && r <= v && got[(size_t)r] == r)) {
            std::printf("%s: labels[%d] = %d is no root at or below it\n", what, (int)v, (int)r);
            failures++;
            break;
        }
    }
}

int main() {
    unsigned char buffer[16] = {0};
    const void *p = buffer;
    const int64_t max_nv = ((int64_t)1 << 31) - 2, max_nf = (((int64_t)1 << 31) - 1) / 3;

    // ---- the verdict: the accepted edges
    EXPECT(components_args(true, 5, 7, p, p) == LAUNCH);
    EXPECT(components_args(true, 5, 0, nullptr, p) == LAUNCH);          // no faces, none read
    EXPECT(components_args(true, 0, 0, nullptr, nullptr) == EMPTY);     // nothing to write
    EXPECT(components_args(true, 0, 7, nullptr, nullptr) == EMPTY);
    EXPECT(components_args(true, max_nv, 1, p, p) == LAUNCH);
    EXPECT(components_args(true, 1, max_nf, p, p) == LAUNCH);
    EXPECT(3 * max_nf <= INT32_LIMIT && 3 * (max_nf + 1) > INT32_LIMIT);
    EXPECT(max_nv + 1 == INT32_LIMIT);
    // ---- every refusal
    EXPECT(status(components_args(false, 5, 7, p, p)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, -1, 7, p, p)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, 5, -1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, max_nv + 1, 1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, 1, max_nf + 1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, 0, max_nf + 1, p, p)) == RN_ERR_INVALID);   // before EMPTY
    EXPECT(status(components_args(true, std::numeric_limits<int64_t>::max(), 1, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(components_args(true, 1, std::numeric_limits<int64_t>::max(), p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(components_args(true, std::numeric_limits<int64_t>::min(), 1, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(components_args(true, 5, 7, p, nullptr)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, 5, 7, nullptr, p)) == RN_ERR_INVALID);
    EXPECT(status(components_args(true, 5, 0, nullptr, nullptr)) == RN_ERR_INVALID);

    // ---- which faces count, and where they lie in `faces`
    EXPECT(face_counts_in(5, 0, 4, 2) && face_counts_in(5, 3, 3, 3) && face_counts_in(1, 0, 0, 0));
    EXPECT(!face_counts_in(5, -1, 4, 2) && !face_counts_in(5, 0, 5, 2) && !face_counts_in(5, 0, 4, 5));
    EXPECT(!face_counts_in(5, 0, 1, std::numeric_limits<int32_t>::max()));
    EXPECT(!face_counts_in(5, std::numeric_limits<int32_t>::min(), 1, 2));
    EXPECT(!face_counts_in(0, 0, 0, 0));
    EXPECT(face_counts_in(max_nv, max_nv - 1, 0, 0) && !face_counts_in(max_nv, max_nv, 0, 0));
    EXPECT(face_index(0, 0) == 0 && face_index(1, 0) == 3 && face_index(max_nf - 1, 2) == 3 * (size_t)max_nf - 1);
    EXPECT(face_index(max_nf - 1, 2) <= (size_t)INT32_LIMIT - 1);
    // ---- the launch geometry: at least one block, at most MAX_BLOCKS, the rest is the stride
    EXPECT(blocks(0, 256) == 1 && blocks(1, 256) == 1 && blocks(256, 256) == 1 && blocks(257, 256) == 2);
    EXPECT(blocks(2048 * 256, 256) == 2048 && blocks(2048 * 256 + 1, 256) == 2048);
    EXPECT(blocks(max_nv, 256) == MAX_BLOCKS && blocks(max_nf, 256) == MAX_BLOCKS);
    EXPECT(step_bound(max_nv) == INT32_LIMIT && step_bound(1) == 2);

    // ---- the union-find: 8 threads against a sequential one
    for (int32_t nv : {1, 2, 3, 64, 65, 256, 257, 20003}) {
        const Mesh s = strip(nv);
        check(s, "strip");
        Mesh r = s;
        for (int32_t &v : r.faces) v = nv - 1 - v;
        check(r, "strip, reversed ids");
        check(shuffled(s, 7u + (unsigned)nv), "strip, shuffled");
    }
    check(star(5000, false), "star at vertex 0");
    check(star(5000, true), "star at the last vertex");
    check(shuffled(star(5000, false), 3u), "star, shuffled");
    check(pieces(400), "pieces");
    check(shuffled(pieces(400), 5u), "pieces, shuffled");
    {
        // two strips joined only by the last face
        Mesh m = strip(4000);
        for (int32_t i = 4000; i + 2 < 8000; i++) m.faces.insert(m.faces.end(), {i, i + 1, i + 2});
        m.nv = 8000;
        bool ok = false;
        EXPECT(concurrent(m, 8, &ok)[7999] == 4000 && ok);
        m.faces.insert(m.faces.end(), {3999, 7999, 4000});
        check(m, "two strips and a bridge");
        EXPECT(concurrent(m, 8, &ok)[7999] == 0 && ok);
    }
    {
        // a chase that is longer than its bound says so (and returns): a hand-made chain, bound 3
        std::vector<int32_t> parent = {0, 0, 1, 2, 3, 4, 5, 6};
        std::vector<int32_t> copy = parent;
        const HostAtomics at{copy.data()};
        bool ok = true;
        find(at, 7, 3, &ok);
        EXPECT(!ok);
        copy = parent;
        ok = true;
        EXPECT(find(at, 7, step_bound(8), &ok) == 0 && ok);
        for (size_t v = 0; v < copy.size(); v++) EXPECT(copy[v] <= (int32_t)v);
        copy = parent;
        EXPECT(!unite(at, 7, 0, 0));
    }
    return finish("components");
}
