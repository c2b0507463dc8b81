// Stand-alone host program over raynet_amd/csrc/raynet_holes_args.h: the refusals of
// rn_mesh_fill_holes and its accepted edges, the workspace layout, and the phases of the kernels
// run as a sequential "GPU" -- every thread index, forwards and backwards, over heap blocks of
// exactly the sizes the entry asks for -- and compared with a std::map implementation of the
// definition written here.  The header holds no HIP, so all of it runs without a GPU.
// tests/test_holes_cpu.py builds it with -fsanitize=address,undefined and runs it; it exits 0 when
// every expectation holds and prints the first one that does not.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_holes_args.h"
#include "host_main.h"

using namespace rn_hl;

static int status_of(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

// the policies on the host: one thread at a time, plain words
struct HostUnion {
    int32_t *parent;
    int32_t load(int32_t x) const { return parent[x]; }
    int32_t cas(int32_t x, int32_t expect, int32_t value) const {
        const int32_t seen = parent[x];
        if (seen == expect) parent[x] = value;
        return seen;
    }
    void store(int32_t x, int32_t value) const { parent[x] = value; }
};
struct HostAtomics {
    void add_i32(int32_t *p, int32_t x) const { *p += x; }
    void min_i32(int32_t *p, int32_t x) const { *p = std::min(*p, x); }
    void add_i64(int64_t *p, int64_t x) const { *p += x; }
};

struct Mesh {
    std::vector<float> vertices;            // [nv][3]
    std::vector<int32_t> faces;             // [nf][3]
    int64_t nv() const { return (int64_t)vertices.size() / 3; }
    int64_t nf() const { return (int64_t)faces.size() / 3; }
};

// a height field over w x h cells without the cells of `removed`; vertex y (w + 1) + x
static Mesh sheet(int w, int h, const std::set<std::pair<int, int>> &removed, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> noise(-0.2f, 0.2f);
    Mesh m;
    for (int y = 0; y <= h; y++)
        for (int x = 0; x <= w; x++)
            m.vertices.insert(m.vertices.end(), {(float)x + noise(rng), (float)y + noise(rng), noise(rng)});
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            if (removed.count({x, y})) continue;
            const int32_t q = y * (w + 1) + x;
            m.faces.insert(m.faces.end(), {q, q + 1, q + w + 2, q, q + w + 2, q + w + 1});
        }
    return m;
}

static Mesh tube(int n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> noise(-0.01f, 0.01f);
    Mesh m;
    for (int ring = 0; ring < 2; ring++)
        for (int i = 0; i < n; i++) {
            const double t = 6.283185307179586 * i / n;
            m.vertices.insert(m.vertices.end(), {(float)std::cos(t) + noise(rng),
                                                 (float)std::sin(t) + noise(rng), (float)ring});
        }
    for (int32_t i = 0; i < n; i++) {
        const int32_t j = (i + 1) % n;
        m.faces.insert(m.faces.end(), {i, j, n + j, i, n + j, n + i});
    }
    return m;
}

static Mesh shuffled_faces(const Mesh &in, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<int64_t> rows((size_t)in.nf());
    std::iota(rows.begin(), rows.end(), 0);
    std::shuffle(rows.begin(), rows.end(), rng);
    Mesh m{in.vertices, {}};
    for (int64_t r : rows)
        for (int k = 0; k < 3; k++) m.faces.push_back(in.faces[xyz_index(r, k)]);
    return m;
}

// the corner table of a mesh whose faces may hold garbage: the corners that name a vertex sorted by
// it, the others behind them
static void corner_table(const Mesh &m, std::vector<int32_t> *offsets, std::vector<int32_t> *corners) {
    const int64_t nv = m.nv();
    offsets->assign((size_t)nv + 1, 0);
    corners->resize(m.faces.size());
    std::iota(corners->begin(), corners->end(), 0);
    auto key = [&](int32_t c) {
        const int64_t v = m.faces[(size_t)c];
        return vertex_in(v, nv) ? v : nv;
    };
    std::stable_sort(corners->begin(), corners->end(),
                     [&](int32_t a, int32_t b) { return key(a) < key(b); });
    for (int32_t v : m.faces)
        if (vertex_in(v, nv)) (*offsets)[(size_t)v + 1]++;
    for (int64_t v = 0; v < nv; v++) (*offsets)[(size_t)v + 1] += (*offsets)[(size_t)v];
}

struct Result {
    bool ok = true;
    std::vector<float> new_vertices;
    std::vector<int32_t> new_faces, source;
    int64_t counts[5] = {0, 0, 0, 0, 0};
};

static bool same(const Result &a, const Result &b) {
    return a.ok == b.ok && a.new_faces == b.new_faces && a.source == b.source &&
           a.new_vertices.size() == b.new_vertices.size() &&
           (a.new_vertices.empty() ||
            !std::memcmp(a.new_vertices.data(), b.new_vertices.data(), 4 * a.new_vertices.size())) &&
           !std::memcmp(a.counts, b.counts, sizeof(a.counts));
}

// ---- the definition, with std::map ----
static Result by_definition(const Mesh &m, int32_t max_edges) {
    const int64_t nv = m.nv(), nf = m.nf();
    std::map<std::pair<int32_t, int32_t>, int> in_faces;
    auto counts_in = [&](int64_t f) {
        return face_counts(nv, m.faces[xyz_index(f, 0)], m.faces[xyz_index(f, 1)], m.faces[xyz_index(f, 2)]);
    };
    for (int64_t f = 0; f < nf; f++)
        if (counts_in(f))
            for (int s = 0; s < 3; s++) {
                const int32_t p = m.faces[xyz_index(f, s)], q = m.faces[xyz_index(f, (s + 1) % 3)];
                in_faces[{std::min(p, q), std::max(p, q)}]++;
            }
    std::vector<std::pair<int32_t, int32_t>> half;
    for (int64_t f = 0; f < nf; f++)
        if (counts_in(f))
            for (int s = 0; s < 3; s++) {
                const int32_t p = m.faces[xyz_index(f, s)], q = m.faces[xyz_index(f, (s + 1) % 3)];
                if (in_faces[{std::min(p, q), std::max(p, q)}] == 1) half.push_back({p, q});
            }
    std::vector<int32_t> parent((size_t)nv);
    std::iota(parent.begin(), parent.end(), 0);
    auto root = [&](int32_t x) {
        while (parent[(size_t)x] != x) x = parent[(size_t)x];
        return x;
    };
    std::map<int32_t, int> out_deg, in_deg;
    std::map<int32_t, int32_t> way_out;
    for (auto [a, b] : half) {
        out_deg[a]++;
        in_deg[b]++;
        way_out.insert({a, b});             // (ascending h: the first stays)
        const int32_t ra = root(a), rb = root(b);
        if (ra != rb) parent[(size_t)std::max(ra, rb)] = std::min(ra, rb);
    }
    std::map<int32_t, int32_t> edges;
    std::set<int32_t> bad;
    for (auto [a, b] : half) {
        const int32_t r = root(a);
        edges[r]++;
        for (int32_t x : {a, b}) {
            bool plain = out_deg[x] == 1 && in_deg[x] == 1;
            for (int k = 0; k < 3; k++) plain = plain && std::isfinite(m.vertices[xyz_index(x, k)]);
            if (!plain) bad.insert(r);
        }
    }
    Result out;
    for (auto [r, E] : edges) {
        if (bad.count(r) || E < 3 || E > max_edges) continue;
        const int32_t k = (int32_t)out.source.size();
        double s[3] = {0.0, 0.0, 0.0};
        int32_t x = r;
        for (int32_t j = 0; j < E; j++) {
            for (int a = 0; a < 3; a++) s[a] = s[a] + (double)m.vertices[xyz_index(x, a)];
            out.new_faces.insert(out.new_faces.end(), {way_out[x], x, (int32_t)nv + k});
            x = way_out[x];
        }
        if (x != r) out.ok = false;
        for (int a = 0; a < 3; a++) out.new_vertices.push_back((float)(s[a] / (double)E));
        out.source.push_back(r);
    }
    out.counts[0] = (int64_t)out.source.size();
    out.counts[1] = (int64_t)out.new_faces.size() / 3;
    out.counts[2] = (int64_t)edges.size();
    out.counts[3] = (int64_t)bad.size();
    out.counts[4] = (int64_t)half.size();
    return out;
}

// ---- the kernels' phases, one "thread" after the other, in either order; every buffer a heap block
// of exactly the size the entry asks for, the outputs prefilled ----
template <class Fn>
static void launch(int64_t n, bool backwards, Fn fn) {
    for (int64_t i = 0; i < n; i++) fn(backwards ? n - 1 - i : i);
}

static Result by_phases(const Mesh &m, const std::vector<int32_t> &offsets,
                        const std::vector<int32_t> &corners, int32_t max_edges, bool backwards) {
    const int64_t nv = m.nv(), nf = m.nf();
    const int64_t bytes = workspace_bytes(nv, nf);
    EXPECT(bytes > 0 && bytes % 8 == 0);
    std::unique_ptr<uint64_t[]> workspace(new uint64_t[(size_t)bytes / 8]);
    std::memset(workspace.get(), 0xa5, (size_t)bytes);
    std::unique_ptr<float[]> new_vertices(new float[3 * (size_t)nf]);
    std::unique_ptr<int32_t[]> new_faces(new int32_t[9 * (size_t)nf]), source(new int32_t[(size_t)nf]);
    std::fill_n(new_vertices.get(), 3 * nf, -7.0f);
    std::fill_n(new_faces.get(), 9 * nf, -7);
    std::fill_n(source.get(), nf, -7);
    // exactly-sized copies of the inputs, so that a read beyond them is caught too
    std::unique_ptr<float[]> v(new float[3 * (size_t)nv]);
    std::unique_ptr<int32_t[]> f(new int32_t[3 * (size_t)nf]), off(new int32_t[(size_t)nv + 1]),
        cor(new int32_t[3 * (size_t)nf]);
    std::copy(m.vertices.begin(), m.vertices.end(), v.get());
    std::copy(m.faces.begin(), m.faces.end(), f.get());
    std::copy(offsets.begin(), offsets.end(), off.get());
    std::copy(corners.begin(), corners.end(), cor.get());
    Result out;
    EXPECT(fill_args(true, nv, v.get(), nf, f.get(), off.get(), cor.get(), max_edges,
                     new_vertices.get(), new_faces.get(), source.get(), out.counts,
                     workspace.get()) == LAUNCH);
    const Tables t = tables_of(nv, nf, max_edges, workspace.get());
    const HostAtomics at{};
    const HostUnion uf{t.parent};
    launch(nv, backwards, [&](int64_t i) { init_vertex(i, t); });
    launch(3 * nf, backwards, [&](int64_t h) {
        if (!mark_edge(at, uf, h, f.get(), off.get(), cor.get(), t)) out.ok = false;
    });
    for (int64_t i = 0; i < nv; i++) EXPECT(t.parent[i] <= i);
    launch(nv, backwards, [&](int64_t i) {
        if (!rn_cc::flatten(uf, (int32_t)i, rn_cc::step_bound(nv))) out.ok = false;
    });
    launch(3 * nf, backwards, [&](int64_t h) { tally_edge(at, h, v.get(), f.get(), t); });
    std::memset(t.partial, 0, (size_t)partial_bytes());     // (the launcher's hipMemsetAsync)
    launch(nv, backwards, [&](int64_t i) { flag_vertex(at, i, t, (int)(i / 256 % SLOTS)); });
    uint64_t sum = 0;                       // the exclusive scan
    for (int64_t i = 0; i < nv; i++) {
        const uint64_t word = t.scan[i];
        t.scan[i] = sum;
        sum += word;
    }
    t.total[0] = sum;
    launch(nv, backwards, [&](int64_t i) {
        if (!emit_loop(i, v.get(), f.get(), t, out.counts, new_vertices.get(), new_faces.get(),
                       source.get()))
            out.ok = false;
    });
    if (t.status[0] != 0) out.ok = false;
    // the inputs are untouched, the rows beyond the counts keep their prefill
    EXPECT(std::equal(m.vertices.begin(), m.vertices.end(), v.get(),
                      [](float a, float b) { return !std::memcmp(&a, &b, 4); }));
    EXPECT(std::equal(m.faces.begin(), m.faces.end(), f.get()));
    const int64_t k = out.counts[0], n = out.counts[1];
    EXPECT(k >= 0 && k <= nf && n >= 0 && n <= 3 * nf);
    for (int64_t i = 3 * k; i < 3 * nf; i++) EXPECT(new_vertices[(size_t)i] == -7.0f);
    for (int64_t i = 3 * n; i < 9 * nf; i++) EXPECT(new_faces[(size_t)i] == -7);
    for (int64_t i = k; i < nf; i++) EXPECT(source[(size_t)i] == -7);
    out.new_vertices.assign(new_vertices.get(), new_vertices.get() + 3 * k);
    out.new_faces.assign(new_faces.get(), new_faces.get() + 3 * n);
    out.source.assign(source.get(), source.get() + k);
    return out;
}

static Result check(const Mesh &m, int32_t max_edges, const char *what) {
    std::vector<int32_t> offsets, corners;
    corner_table(m, &offsets, &corners);
    const Result want = by_definition(m, max_edges);
    for (bool backwards : {false, true}) {
        const Result got = by_phases(m, offsets, corners, max_edges, backwards);
        if (!got.ok || !same(got, want)) {
            std::printf("%s (max_edges %d, %s): %s\n", what, (int)max_edges,
                        backwards ? "backwards" : "forwards",
                        got.ok ? "differs from the definition" : "a bound was reached");
            failures++;
        }
    }
    return want;
}

int main() {
    alignas(8) unsigned char buffer[8192] = {0};
    const int64_t max_nv = ((int64_t)1 << 31) - 2, max_nf = (((int64_t)1 << 31) - 1) / 3;
    // eight disjoint blocks for the nine arrays of a mesh of 4 vertices and 4 faces (faces and
    // corners, both inputs, may share one)
    const int64_t nv = 4, nf = 4;
    unsigned char *vp = buffer, *fp = buffer + 64, *op = buffer + 128, *cp = buffer + 192,
                  *nvp = buffer + 256, *nfp = buffer + 320, *sp = buffer + 480, *kp = buffer + 512,
                  *wp = buffer + 1024;
    EXPECT(workspace_bytes(nv, nf) <= 7168);
    auto verdict = [&](int64_t a_nv, int64_t a_nf, int32_t max_edges) {
        return fill_args(true, a_nv, vp, a_nf, fp, op, cp, max_edges, nvp, nfp, sp, kp, wp);
    };
    // ---- the verdict: the accepted edges
    EXPECT(verdict(nv, nf, 3) == LAUNCH && verdict(nv, nf, 65536) == LAUNCH);
    EXPECT(fill_args(true, nv, vp, nf, fp, op, fp, 3, nvp, nfp, sp, kp, wp) == LAUNCH);
    EXPECT(fill_args(true, 0, nullptr, 0, nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr,
                     kp, nullptr) == EMPTY);
    EXPECT(fill_args(true, 0, nullptr, 7, nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr,
                     kp, nullptr) == EMPTY);
    EXPECT(fill_args(true, 7, nullptr, 0, nullptr, nullptr, nullptr, 3, nullptr, nullptr, nullptr,
                     kp, nullptr) == EMPTY);
    EXPECT(fill_sizes_ok(max_nv, 0) && fill_sizes_ok(0, max_nf) && fill_sizes_ok(max_nv - 5, 5));
    // ---- every refusal
    EXPECT(status_of(fill_args(false, nv, vp, nf, fp, op, cp, 3, nvp, nfp, sp, kp, wp)) == RN_ERR_INVALID);
    EXPECT(status_of(verdict(-1, nf, 3)) == RN_ERR_INVALID && status_of(verdict(nv, -1, 3)) == RN_ERR_INVALID);
    EXPECT(!fill_sizes_ok(max_nv + 1, 0) && !fill_sizes_ok(0, max_nf + 1));
    EXPECT(!fill_sizes_ok(max_nv - 5, 6) && !fill_sizes_ok(max_nv, 1));    // nv + nf is an int32
    EXPECT(!fill_sizes_ok(std::numeric_limits<int64_t>::max(), 1));
    EXPECT(!fill_sizes_ok(1, std::numeric_limits<int64_t>::max()));
    EXPECT(!fill_sizes_ok(std::numeric_limits<int64_t>::min(), 1));
    EXPECT(workspace_bytes(-1, 0) == -1 && workspace_bytes(max_nv + 1, 0) == -1);
    EXPECT(workspace_bytes(0, max_nf + 1) == -1 && workspace_bytes(max_nv, 1) == -1);
    for (int32_t bad : {2, 0, -1, 65537, std::numeric_limits<int32_t>::max(),
                        std::numeric_limits<int32_t>::min()})
        EXPECT(status_of(verdict(nv, nf, bad)) == RN_ERR_INVALID);
    EXPECT(status_of(fill_args(true, 0, nullptr, 0, nullptr, nullptr, nullptr, 2, nullptr, nullptr,
                               nullptr, kp, nullptr)) == RN_ERR_INVALID);       // before EMPTY
    EXPECT(status_of(fill_args(true, 0, nullptr, 0, nullptr, nullptr, nullptr, 3, nullptr, nullptr,
                               nullptr, nullptr, nullptr)) == RN_ERR_INVALID);  // counts
    {
        const void *args[9] = {vp, fp, op, cp, nvp, nfp, sp, kp, wp};
        for (int null_at = 0; null_at < 9; null_at++) {
            const void *a[9];
            std::copy(args, args + 9, a);
            a[null_at] = nullptr;
            EXPECT(status_of(fill_args(true, nv, a[0], nf, a[1], a[2], a[3], 3, a[4], a[5], a[6],
                                       a[7], a[8])) == RN_ERR_INVALID);
        }
        // an output that shares a byte with an input or another output: its first byte, its last
        for (int out_at = 4; out_at < 9; out_at++)
            for (int other = 0; other < 9; other++) {
                if (other == out_at) continue;
                const void *a[9];
                std::copy(args, args + 9, a);
                a[out_at] = args[other];
                if (out_at == 8 && (uintptr_t)a[8] % 8 != 0) continue;
                EXPECT(status_of(fill_args(true, nv, a[0], nf, a[1], a[2], a[3], 3, a[4], a[5],
                                           a[6], a[7], a[8])) == RN_ERR_INVALID);
            }
        EXPECT(status_of(fill_args(true, nv, vp, nf, fp, op, cp, 3, kp + 8 * COUNTS - 1, nfp, sp, kp, wp)) ==
               RN_ERR_INVALID);
        EXPECT(fill_args(true, nv, vp, nf, fp, op, cp, 3, kp + 8 * COUNTS, nfp, sp, kp, wp) == LAUNCH);
        EXPECT(status_of(fill_args(true, nv, vp, nf, fp, op, cp, 3, nvp, nfp, sp, kp, wp + 4)) ==
               RN_ERR_INVALID);                                                 // alignment
        EXPECT(status_of(fill_args(true, nv, vp, nf, fp, op, cp, 3, nvp, nfp, sp, kp, wp + 1)) ==
               RN_ERR_INVALID);
    }
    EXPECT(overlap(vp, 4, vp + 3, 4) && !overlap(vp, 4, vp + 4, 4) && !overlap(vp, 0, vp, 4));

    // ---- the workspace: 64-bit words first, every array behind the one in front, 8-byte ends
    for (int64_t a_nv : {1, 2, 255, 256, 257, 65536, 65537, 100000})
        for (int64_t a_nf : {1, 3, 170, 200001}) {
            const int64_t words = rn_scan::scan_scratch_words(a_nv);
            EXPECT(ws_scan(a_nv, a_nf) == 0 && ws_scratch(a_nv, a_nf) == 8 * a_nv);
            EXPECT(ws_total(a_nv, a_nf) == 8 * (a_nv + words));
            EXPECT(ws_partial(a_nv, a_nf) == ws_total(a_nv, a_nf) + 8);
            EXPECT(ws_parent(a_nv, a_nf) == ws_partial(a_nv, a_nf) + 8 * 3 * SLOTS);
            EXPECT(ws_out_deg(a_nv, a_nf) - ws_parent(a_nv, a_nf) == 4 * a_nv);
            EXPECT(ws_in_deg(a_nv, a_nf) - ws_out_deg(a_nv, a_nf) == 4 * a_nv);
            EXPECT(ws_out_edge(a_nv, a_nf) - ws_in_deg(a_nv, a_nf) == 4 * a_nv);
            EXPECT(ws_edges(a_nv, a_nf) - ws_out_edge(a_nv, a_nf) == 4 * a_nv);
            EXPECT(ws_bad(a_nv, a_nf) - ws_edges(a_nv, a_nf) == 4 * a_nv);
            EXPECT(ws_status(a_nv, a_nf) - ws_bad(a_nv, a_nf) == 4 * a_nv);
            EXPECT(ws_boundary(a_nv, a_nf) == ws_status(a_nv, a_nf) + 8);
            const int64_t bytes = workspace_bytes(a_nv, a_nf);
            EXPECT(bytes % 8 == 0 && bytes >= ws_boundary(a_nv, a_nf) + 3 * a_nf &&
                   bytes < ws_boundary(a_nv, a_nf) + 3 * a_nf + 8);
            EXPECT(ws_total(a_nv, a_nf) % 8 == 0 && ws_parent(a_nv, a_nf) % 8 == 0);
        }
    EXPECT(workspace_bytes(257, 255) == (8 * 257 + 8 * 2 + 8 + 6144 + 24 * 257 + 8 + 3 * 255 + 7) / 8 * 8);
    EXPECT(workspace_bytes(0, 0) == 16 + 6144 && partial_bytes() == 6144 && SLOTS == 256);

    // ---- the pieces
    EXPECT(face_counts(5, 0, 4, 2) && !face_counts(5, 3, 3, 3) && !face_counts(5, 0, 1, 0));
    EXPECT(!face_counts(5, 0, 0, 1) && !face_counts(5, 1, 0, 0) && !face_counts(5, -1, 4, 2));
    EXPECT(!face_counts(5, 0, 5, 2) && !face_counts(5, 0, 1, std::numeric_limits<int32_t>::max()));
    EXPECT(finite(0.0f) && finite(-1e38f) && finite(std::numeric_limits<float>::denorm_min()));
    EXPECT(!finite(std::numeric_limits<float>::infinity()) && !finite(-std::numeric_limits<float>::infinity()));
    EXPECT(!finite(std::numeric_limits<float>::quiet_NaN()));
    EXPECT(scan_word(3) == (((uint64_t)1 << 32) | 3) && word_loops(scan_word(65536)) == 1);
    EXPECT(word_faces(scan_word(65536)) == 65536);
    EXPECT(word_loops(715827882ull * scan_word(3)) == 715827882 &&
           word_faces(715827882ull * scan_word(3)) == 3 * max_nf);      // the low half never carries
    EXPECT(blocks(3 * max_nf, 256) == MAX_BLOCKS && blocks(0, 256) == 1);

    // ---- the phases against the definition
    {
        Mesh tetra{{0, 0, 1, 1, 0, 0, -0.5f, 0.75f, 0, -0.5f, -0.75f, 0.125f}, {0, 1, 2, 0, 2, 3, 0, 3, 1}};
        const Result r = check(tetra, 3, "open tetrahedron");
        EXPECT(r.counts[0] == 1 && r.counts[1] == 3 && r.counts[4] == 3 && r.source[0] == 1);
        EXPECT((r.new_faces == std::vector<int32_t>{2, 1, 4, 3, 2, 4, 1, 3, 4}));
        tetra.faces.insert(tetra.faces.end(), {1, 3, 2});
        EXPECT(check(tetra, 3, "closed tetrahedron").counts[2] == 0);
    }
    for (int n : {3, 63, 64, 65, 300}) {
        const Mesh t = tube(n, 11u);
        const Result r = check(t, n, "tube");
        EXPECT(r.counts[0] == 2 && r.counts[1] == 2 * n && r.counts[2] == 2 && r.counts[3] == 0);
        EXPECT(r.source[0] == 0 && r.source[1] == n);
        if (n > 3) EXPECT(check(t, n - 1, "tube, too long").counts[0] == 0);
        check(shuffled_faces(t, 5u), n, "tube, shuffled");
    }
    const std::set<std::pair<int, int>> punched = {{2, 2}, {3, 2}, {6, 5}, {9, 3}, {9, 4}};
    const Mesh holes = sheet(12, 9, punched, 1u);
    {
        const Result r = check(holes, 10, "punched sheet");
        EXPECT(r.counts[0] == 3 && r.counts[1] == 16 && r.counts[2] == 4 && r.counts[3] == 0 &&
               r.counts[4] == 58);
        EXPECT((r.source == std::vector<int32_t>{28, 48, 71}));
        EXPECT(check(holes, 3, "punched sheet, triangles only").counts[0] == 0);
        EXPECT(check(holes, 41, "punched sheet, 41").counts[0] == 3);
        EXPECT(check(holes, 42, "punched sheet, 42").counts[0] == 4);
        EXPECT(check(holes, 65536, "punched sheet, 65536").counts[1] == 58);
        check(shuffled_faces(holes, 9u), 10, "punched sheet, shuffled");
    }
    {
        const Result r = check(sheet(8, 8, {{2, 2}, {3, 3}, {6, 1}}, 2u), 10, "bow-tie");
        EXPECT(r.counts[0] == 1 && r.counts[2] == 3 && r.counts[3] == 1 && r.source[0] == 15);
        EXPECT(check(sheet(8, 8, {{2, 2}, {3, 3}, {6, 1}}, 2u), 65536, "bow-tie, any").counts[0] == 2);
    }
    {
        // the face (70, 71, 84) at the hole of cell (6, 5): turned over, doubled; a NaN at vertex 72
        Mesh m = holes;
        int64_t row = -1;
        for (int64_t f = 0; f < m.nf(); f++)
            if (m.faces[xyz_index(f, 0)] == 70 && m.faces[xyz_index(f, 1)] == 71 &&
                m.faces[xyz_index(f, 2)] == 84)
                row = f;
        EXPECT(row >= 0);
        std::swap(m.faces[xyz_index(row, 0)], m.faces[xyz_index(row, 2)]);
        Result r = check(m, 10, "flipped rim");
        EXPECT(r.counts[0] == 2 && r.counts[3] == 1 && (r.source == std::vector<int32_t>{28, 48}));
        m = holes;
        m.faces.insert(m.faces.end(), {70, 71, 84});
        r = check(m, 10, "doubled face");
        EXPECT(r.counts[0] == 2 && r.counts[3] == 1 && r.counts[4] == 16 - 4 + 42 + 3);
        m = holes;
        m.vertices[xyz_index(72, 1)] = std::numeric_limits<float>::quiet_NaN();
        r = check(m, 10, "NaN rim");
        EXPECT(r.counts[0] == 2 && r.counts[3] == 1 && r.counts[4] == 58);
        m.vertices[xyz_index(72, 1)] = std::numeric_limits<float>::infinity();
        EXPECT(check(m, 10, "infinite rim").counts[3] == 1);
        // faces that do not count change nothing
        m = holes;
        m.faces.insert(m.faces.begin() + 30, {0, 1, 130, -1, 2, 3, 4, 4, 5});
        m.faces.insert(m.faces.end(), {6, 7, 6, std::numeric_limits<int32_t>::max(), 0, 1,
                                       std::numeric_limits<int32_t>::min(), 1, 2, 3, 3, 3});
        r = check(m, 10, "garbage");
        const Result clean = by_definition(holes, 10);
        EXPECT(same(r, clean));
    }
    {
        // more filled loops than one tile of the scan holds
        std::set<std::pair<int, int>> raster;
        for (int x = 2; x < 69; x += 2)
            for (int y = 2; y < 69; y += 2) raster.insert({x, y});
        const Mesh m = sheet(70, 70, raster, 4u);
        const Result r = check(m, 16, "raster");
        EXPECT(r.counts[0] == 34 * 34 && r.counts[1] == 4 * 34 * 34 && r.counts[2] == 34 * 34 + 1);
        check(shuffled_faces(m, 6u), 16, "raster, shuffled");
    }
    {
        // a corner table that is not the mesh's: nothing out of bounds, no bound reached, and the
        // counts stay within the outputs (by_phases checks that)
        std::vector<int32_t> offsets, corners;
        corner_table(holes, &offsets, &corners);
        std::mt19937 rng(13u);
        const int32_t junk[] = {-1, (int32_t)(3 * holes.nf()), std::numeric_limits<int32_t>::max(),
                                std::numeric_limits<int32_t>::min(), 0, 17};
        for (int round = 0; round < 20; round++) {
            std::vector<int32_t> off = offsets, cor = corners;
            for (size_t i = 0; i < off.size(); i++)
                if (rng() % 10 == 0) off[i] = junk[rng() % 6];
            for (size_t i = 0; i < cor.size(); i++)
                if (rng() % 10 == 0) cor[i] = junk[rng() % 6];
            for (bool backwards : {false, true})
                EXPECT(by_phases(holes, off, cor, 10, backwards).ok);
        }
    }
    return finish("holes");
}
