// simplify_args_main.cpp -- raynet_simplify_args.h on the host, under the address and
// undefined-behaviour sanitizers (tests/test_simplify_cpu.py builds and runs this program):
//   * the verdict of rn_mesh_simplify's arguments at every limit and one beyond it;
//   * the workspace layout: no overlap, the 64-bit parts 8-byte aligned;
//   * whole simplifications as the launcher's own sequence of phases, executed serially over the
//     header's functions, every buffer a heap block of exactly the size the definition names, each
//     result compared bit for bit with a second, straightforward implementation (a std::map from
//     cell to members, std::floor and std::rint).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <random>
#include <vector>

#include "raynet_simplify_args.h"
#include "host_main.h"

using namespace rn_sp;

// ------------------------------------------------------------------------------ the verdict
static void test_verdict() {
    const double origin[3] = {0.0, -1.0, 2.5}, cell[3] = {1.0, 0.5, 2.0};
    const int32_t dims[3] = {4, 5, 6};
    alignas(8) char block[64];
    const void *vin = block, *vout = block + 8, *fin = block + 16, *fout = block + 24,
               *counts = block + 32, *ws = block + 40;
    auto verdict = [&](int64_t nv, int64_t nf) {
        return simplify_args(true, nv, vin, nf, fin, origin, cell, dims, vout, fout, counts, ws);
    };
    const int64_t NV = ((int64_t)1 << 31) - 2, NF = (((int64_t)1 << 31) - 1) / 3;
    EXPECT(verdict(3, 1) == LAUNCH);
    EXPECT(verdict(NV, NF) == LAUNCH);
    EXPECT(verdict(NV + 1, 1) == INVALID);
    EXPECT(verdict(3, NF + 1) == INVALID);
    EXPECT(3 * NF <= ((int64_t)1 << 31) - 1 && 3 * (NF + 1) > ((int64_t)1 << 31) - 1);
    EXPECT(verdict(-1, 0) == INVALID && verdict(0, -1) == INVALID);
    EXPECT(verdict(0, 0) == EMPTY && verdict(0, 5) == EMPTY);
    EXPECT(simplify_args(false, 3, vin, 1, fin, origin, cell, dims, vout, fout, counts, ws) == INVALID);
    // nv == 0: whatever the device pointers, but not with bad scalars and not without counts
    EXPECT(simplify_args(true, 0, nullptr, 0, nullptr, origin, cell, dims, nullptr, nullptr, counts,
                         nullptr) == EMPTY);
    EXPECT(simplify_args(true, 0, nullptr, 0, nullptr, origin, cell, dims, nullptr, nullptr, nullptr,
                         nullptr) == INVALID);
    {
        const double bad[3] = {1.0, 0.0, 1.0};
        EXPECT(simplify_args(true, 0, nullptr, 0, nullptr, origin, bad, dims, nullptr, nullptr,
                             counts, nullptr) == INVALID);
        const int32_t none[3] = {4, 0, 6};
        EXPECT(simplify_args(true, 0, nullptr, 0, nullptr, origin, cell, none, nullptr, nullptr,
                             counts, nullptr) == INVALID);
    }
    // dims: every axis, the product at 2^31 - 1 and at 2^31
    for (int k = 0; k < 3; k++)
        for (int32_t bad : {0, -1, std::numeric_limits<int32_t>::min()}) {
            int32_t d[3] = {4, 5, 6};
            d[k] = bad;
            EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, d, vout, fout, counts, ws) == INVALID);
            EXPECT(workspace_bytes(3, 1, d) == -1);
        }
    {
        const int32_t most[3] = {2147483647, 1, 1}, prime[3] = {1, 2147483647, 1};
        const int32_t over[3] = {65536, 32768, 1}, wide[3] = {2147483647, 2147483647, 2147483647};
        const int32_t under[3] = {46340, 46340, 1}, last[3] = {1, 1, 2147483647};
        for (const int32_t *d : {most, prime, under, last}) {
            EXPECT(cell_count(d) > 0 && cell_count(d) <= INT32_LIMIT);
            EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, d, vout, fout, counts, ws) == LAUNCH);
            EXPECT(workspace_bytes(3, 1, d) >= CELL_BYTES * cell_count(d));
        }
        EXPECT(cell_count(most) == INT32_LIMIT);
        for (const int32_t *d : {over, wide}) {
            EXPECT(cell_count(d) == -1 && workspace_bytes(3, 1, d) == -1);
            EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, d, vout, fout, counts, ws) == INVALID);
        }
        EXPECT((int64_t)over[0] * over[1] == (int64_t)1 << 31);
        EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, nullptr, vout, fout, counts, ws) == INVALID);
        EXPECT(workspace_bytes(3, 1, nullptr) == -1);
    }
    // cell and origin
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double denorm = std::numeric_limits<double>::denorm_min();
    for (int k = 0; k < 3; k++) {
        for (double bad : {0.0, -0.0, -1.0, inf, -inf, nan}) {
            double c[3] = {1.0, 0.5, 2.0};
            c[k] = bad;
            EXPECT(simplify_args(true, 3, vin, 1, fin, origin, c, dims, vout, fout, counts, ws) == INVALID);
        }
        for (double good : {denorm, 1e300, std::numeric_limits<double>::max()}) {
            double c[3] = {1.0, 0.5, 2.0};
            c[k] = good;
            EXPECT(simplify_args(true, 3, vin, 1, fin, origin, c, dims, vout, fout, counts, ws) == LAUNCH);
        }
        for (double bad : {inf, -inf, nan}) {
            double o[3] = {0.0, -1.0, 2.5};
            o[k] = bad;
            EXPECT(simplify_args(true, 3, vin, 1, fin, o, cell, dims, vout, fout, counts, ws) == INVALID);
        }
    }
    EXPECT(simplify_args(true, 3, vin, 1, fin, nullptr, cell, dims, vout, fout, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, nullptr, dims, vout, fout, counts, ws) == INVALID);
    // each pointer
    EXPECT(simplify_args(true, 3, nullptr, 1, fin, origin, cell, dims, vout, fout, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, nullptr, origin, cell, dims, vout, fout, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, nullptr, fout, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vout, nullptr, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vout, fout, nullptr, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vout, fout, counts, nullptr) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 0, nullptr, origin, cell, dims, vout, nullptr, counts, ws) == LAUNCH);
    // the alignment
    for (int off = 1; off < 8; off++)
        EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vout, fout, counts,
                             block + 40 + off) == INVALID);
    // the aliasings
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vin, fout, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vout, fin, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, ws, fout, counts, ws) == INVALID);
    EXPECT(simplify_args(true, 3, vin, 1, fin, origin, cell, dims, vout, ws, counts, ws) == INVALID);
}

// ------------------------------------------------------------------------------- the layout
static void test_layout() {
    const int32_t shapes[][3] = {{1, 1, 1}, {3, 5, 7}, {64, 64, 64}, {2147483647, 1, 1}};
    const int64_t sizes[][2] = {{1, 0}, {1, 1}, {3, 1}, {257, 255}, {65537, 131070},
                                {((int64_t)1 << 31) - 2, (((int64_t)1 << 31) - 1) / 3}};
    for (auto &d : shapes)
        for (auto &s : sizes) {
            const int64_t nv = s[0], nf = s[1], cells = cell_count(d);
            const int64_t words = rn_scan::scan_scratch_words(nv > nf ? nv : nf);
            const int64_t parts[][2] = {{ws_table(nv, nf, cells), CELL_BYTES * cells},
                                        {ws_fscan(nv, nf, cells), 8 * nf},
                                        {ws_vscan(nv, nf, cells), 8 * nv},
                                        {ws_scratch(nv, nf, cells), 8 * words},
                                        {ws_cell_of(nv, nf, cells), 4 * nv}};
            int64_t at = 0;
            for (int i = 0; i < 5; i++) {
                EXPECT(parts[i][0] == at);                   // one behind the other: no overlap
                if (i < 4) EXPECT(parts[i][0] % 8 == 0);     // the u64 parts
                at += parts[i][1];
            }
            const int64_t bytes = workspace_bytes(nv, nf, d);
            EXPECT(bytes >= at && bytes < at + 8 && bytes % 8 == 0);
        }
    EXPECT(workspace_bytes(-1, 0, shapes[0]) == -1 && workspace_bytes(0, -1, shapes[0]) == -1);
    EXPECT(workspace_bytes(((int64_t)1 << 31) - 1, 0, shapes[0]) == -1);
    EXPECT(workspace_bytes(1, (((int64_t)1 << 31) - 1) / 3 + 1, shapes[0]) == -1);
    EXPECT(workspace_bytes(0, 0, shapes[0]) == 32);
    EXPECT(blocks(0, 256) == 1 && blocks(257, 256) == 2 && blocks((int64_t)1 << 40, 256) == MAX_BLOCKS);
}

// ------------------------------------------------------------------- whole simplifications
struct Mesh {
    std::vector<float> v;       // [nv][3]
    std::vector<int32_t> f;     // [nf][3]
    int64_t nv() const { return (int64_t)v.size() / 3; }
    int64_t nf() const { return (int64_t)f.size() / 3; }
};
struct Space {
    double origin[3], cell[3];
    int32_t dims[3];
};
struct Result {
    std::vector<uint32_t> v;    // the bits
    std::vector<int32_t> f, source, cluster;
    bool operator==(const Result &o) const {
        return v == o.v && f == o.f && source == o.source && cluster == o.cluster;
    }
};

static uint32_t bits_of(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}

// the atomics policy of a serial run
struct SerialAtomics {
    void min_i32(int32_t *p, int32_t x) const { if (x < *p) *p = x; }
    void add_i32(int32_t *p, int32_t x) const { *p += x; }
    void add_u64(uint64_t *p, uint64_t x) const { *p += x; }
};

static uint64_t scan_serial(uint64_t *data, int64_t n) {
    uint64_t sum = 0;
    for (int64_t i = 0; i < n; i++) {
        const uint64_t x = data[i];
        data[i] = sum;
        sum += x;
    }
    return sum;
}

// the launcher's phases over the header's functions, in exactly-sized heap blocks; `order`: the
// order in which the "threads" of the binning and flagging phases run
static Result run_header(const Mesh &m, const Space &s, bool reversed) {
    const int64_t nv = m.nv(), nf = m.nf();
    const float PRE = -12345.5f;
    std::unique_ptr<float[]> vin(new float[3 * nv]), vout(new float[3 * nv]);
    std::unique_ptr<int32_t[]> fin(new int32_t[3 * nf]), fout(new int32_t[3 * nf]);
    std::unique_ptr<int32_t[]> source(new int32_t[nv]), cluster(new int32_t[nv]);
    std::unique_ptr<int64_t[]> counts(new int64_t[2]);
    std::copy(m.v.begin(), m.v.end(), vin.get());
    std::copy(m.f.begin(), m.f.end(), fin.get());
    std::fill(vout.get(), vout.get() + 3 * nv, PRE);
    std::fill(fout.get(), fout.get() + 3 * nf, -77);
    std::fill(source.get(), source.get() + nv, -77);
    std::fill(cluster.get(), cluster.get() + nv, -77);
    const int64_t bytes = workspace_bytes(nv, nf, s.dims);
    EXPECT(bytes >= 0);
    std::unique_ptr<char[]> ws(new char[bytes]);
    std::memset(ws.get(), 0xA5, (size_t)bytes);
    Result r;
    const Verdict verdict = simplify_args(true, nv, vin.get(), nf, fin.get(), s.origin, s.cell,
                                          s.dims, vout.get(), fout.get(), counts.get(), ws.get());
    counts[0] = counts[1] = 0;
    if (verdict == EMPTY) return r;
    EXPECT(verdict == LAUNCH);
    if (nf == 0) {
        r.cluster.assign(nv, -1);
        return r;
    }
    const Grid g = grid_of(s.origin, s.cell, s.dims);
    const Tables t = tables_of(nv, nf, g.cells, ws.get());
    const SerialAtomics at{};
    for (int64_t c = 0; c < g.cells; c++) clear_cell(c, t);
    for (int64_t i = 0; i < nv; i++) bin_vertex(at, reversed ? nv - 1 - i : i, vin.get(), g, t);
    for (int64_t i = 0; i < nf; i++) flag_face(reversed ? nf - 1 - i : i, fin.get(), t, g.cells);
    counts[1] = (int64_t)scan_serial(t.fscan, nf);
    counts[0] = (int64_t)scan_serial(t.vscan, nv);
    for (int64_t i = 0; i < nv; i++)
        emit_vertex(reversed ? nv - 1 - i : i, vin.get(), g, t, counts.get(), vout.get(),
                    source.get(), cluster.get());
    for (int64_t i = 0; i < nf; i++) emit_face(reversed ? nf - 1 - i : i, fin.get(), t, g.cells, fout.get());
    const int64_t nvo = counts[0], nfo = counts[1];
    EXPECT(nvo >= 0 && nvo <= nv && nfo >= 0 && nfo <= nf);
    for (int64_t i = 3 * nvo; i < 3 * nv; i++) EXPECT(bits_of(vout[i]) == bits_of(PRE));
    for (int64_t i = nvo; i < nv; i++) EXPECT(source[i] == -77);
    for (int64_t i = 3 * nfo; i < 3 * nf; i++) EXPECT(fout[i] == -77);
    EXPECT(std::equal(m.v.begin(), m.v.end(), vin.get(),
                      [](float a, float b) { return bits_of(a) == bits_of(b); }));
    EXPECT(std::equal(m.f.begin(), m.f.end(), fin.get()));
    for (int64_t i = 0; i < 3 * nvo; i++) r.v.push_back(bits_of(vout[i]));
    r.f.assign(fout.get(), fout.get() + 3 * nfo);
    r.source.assign(source.get(), source.get() + nvo);
    r.cluster.assign(cluster.get(), cluster.get() + nv);
    // NULL source and cluster: the same vertices and faces
    std::fill(vout.get(), vout.get() + 3 * nv, PRE);
    for (int64_t i = 0; i < nv; i++)
        emit_vertex(i, vin.get(), g, t, counts.get(), vout.get(), nullptr, nullptr);
    for (int64_t i = 0; i < 3 * nvo; i++) EXPECT(bits_of(vout[i]) == r.v[(size_t)i]);
    return r;
}

// the definition again, straightforwardly: a map from cell to members
static Result run_map(const Mesh &m, const Space &s) {
    const int64_t nv = m.nv(), nf = m.nf();
    struct Cell {
        std::vector<int64_t> members;
        int64_t q[3];
    };
    std::map<int64_t, Cell> cells;
    std::vector<int64_t> cell_of(nv, -1), key(nv);
    for (int64_t v = 0; v < nv; v++) {
        int64_t q[3];
        bool binned = true;
        for (int k = 0; k < 3; k++) {
            const double t = ((double)m.v[3 * v + k] - s.origin[k]) / s.cell[k];
            const double fl = std::floor(t);
            if (!std::isfinite(t) || !(fl >= 0.0) || !(fl < (double)s.dims[k])) {
                binned = false;
                break;
            }
            q[k] = (int64_t)fl;
        }
        key[v] = v;
        if (!binned) continue;
        const int64_t c = (q[0] * s.dims[1] + q[1]) * s.dims[2] + q[2];
        cell_of[v] = c;
        Cell &cell = cells[c];
        cell.members.push_back(v);
        std::copy(q, q + 3, cell.q);
    }
    for (auto &entry : cells)
        for (int64_t v : entry.second.members) key[v] = entry.second.members.front();
    Result r;
    std::vector<char> used(nv, 0);
    std::vector<int64_t> kept;
    for (int64_t f = 0; f < nf; f++) {
        const int64_t a = m.f[3 * f], b = m.f[3 * f + 1], c = m.f[3 * f + 2];
        if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) continue;
        if (key[a] == key[b] || key[b] == key[c] || key[a] == key[c]) continue;
        kept.push_back(f);
        used[key[a]] = used[key[b]] = used[key[c]] = 1;
    }
    std::vector<int32_t> index(nv, -1);
    for (int64_t v = 0; v < nv; v++) {
        if (!used[v]) continue;
        index[v] = (int32_t)r.source.size();
        r.source.push_back((int32_t)v);
        const int64_t c = cell_of[v];
        if (c < 0 || cells[c].members.size() == 1) {
            for (int k = 0; k < 3; k++) r.v.push_back(bits_of(m.v[3 * v + k]));
            continue;
        }
        const Cell &cell = cells[c];
        for (int k = 0; k < 3; k++) {
            uint64_t S = 0;
            for (int64_t u : cell.members) {
                const double t = ((double)m.v[3 * u + k] - s.origin[k]) / s.cell[k];
                S += (uint64_t)std::rint((t - std::floor(t)) * 2097152.0);
            }
            const double mean = (double)S / (double)cell.members.size();
            const double inside = mean / 2097152.0;
            const double at = (double)cell.q[k] + inside;
            const double scaled = s.cell[k] * at;
            r.v.push_back(bits_of((float)(s.origin[k] + scaled)));
        }
    }
    for (int64_t f : kept)
        for (int k = 0; k < 3; k++) r.f.push_back(index[key[m.f[3 * f + k]]]);
    for (int64_t v = 0; v < nv; v++) r.cluster.push_back(index[key[v]]);
    return r;
}

static int cases = 0;
static Result check_case(const Mesh &m, const Space &s) {
    const Result a = run_header(m, s, false), b = run_header(m, s, true), c = run_map(m, s);
    EXPECT(a == c);
    EXPECT(b == c);          // the order of the threads plays no part
    // structure: three different indices per face, every vertex in a face, source ascending
    const int64_t nvo = (int64_t)c.source.size();
    std::vector<char> named(nvo, 0);
    for (size_t i = 0; i < a.f.size(); i += 3) {
        EXPECT(a.f[i] != a.f[i + 1] && a.f[i + 1] != a.f[i + 2] && a.f[i] != a.f[i + 2]);
        for (int k = 0; k < 3; k++) {
            EXPECT(a.f[i + k] >= 0 && a.f[i + k] < nvo);
            if (a.f[i + k] >= 0 && a.f[i + k] < nvo) named[a.f[i + k]] = 1;
        }
    }
    for (int64_t o = 0; o < nvo; o++) EXPECT(named[o]);
    for (int64_t o = 1; o < nvo; o++) EXPECT(a.source[o - 1] < a.source[o]);
    cases++;
    return a;
}

static Mesh strip(int64_t nv, unsigned seed, bool permuted) {
    Mesh m;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> noise(-0.3f, 0.3f);
    for (int64_t v = 0; v < nv; v++) {
        m.v.push_back((float)v * 0.5f + noise(rng));
        m.v.push_back(noise(rng) + 1.0f);
        m.v.push_back(noise(rng) - 2.0f);
    }
    for (int64_t i = 0; i + 2 < nv; i++)
        for (int k = 0; k < 3; k++) m.f.push_back((int32_t)(i + k));
    if (permuted) {
        std::vector<int64_t> order(nv);
        for (int64_t v = 0; v < nv; v++) order[v] = v;
        std::shuffle(order.begin(), order.end(), rng);
        Mesh p = m;
        for (int64_t v = 0; v < nv; v++)
            for (int k = 0; k < 3; k++) p.v[3 * order[v] + k] = m.v[3 * v + k];
        for (auto &i : p.f) i = (int32_t)order[i];
        std::vector<int64_t> faces(m.nf());
        for (int64_t f = 0; f < m.nf(); f++) faces[f] = f;
        std::shuffle(faces.begin(), faces.end(), rng);
        Mesh q = p;
        for (int64_t f = 0; f < m.nf(); f++)
            for (int k = 0; k < 3; k++) q.f[3 * f + k] = p.f[3 * faces[f] + k];
        return q;
    }
    return m;
}

static Mesh star(int nf, unsigned seed, bool hub_last) {
    Mesh m;
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> at(-4.0f, 4.0f);
    const int nv = 2 * nf + 1, hub = hub_last ? nv - 1 : 0;
    for (int i = 0; i < 3 * nv; i++) m.v.push_back(at(rng));
    for (int f = 0; f < nf; f++) {
        const int a = hub_last ? 2 * f : 2 * f + 1;
        m.f.push_back(hub);
        m.f.push_back(a);
        m.f.push_back(a + 1);
    }
    return m;
}

static Space around(const Mesh &m, double cx, double cy, double cz) {
    Space s{{0, 0, 0}, {cx, cy, cz}, {1, 1, 1}};
    for (int k = 0; k < 3; k++) {
        double lo = 0.0, hi = 0.0;
        bool any = false;
        for (int64_t v = 0; v < m.nv(); v++) {
            const double x = m.v[3 * v + k];
            if (!std::isfinite(x)) continue;
            lo = any ? std::min(lo, x) : x;
            hi = any ? std::max(hi, x) : x;
            any = true;
        }
        s.origin[k] = std::floor(lo / s.cell[k]) * s.cell[k];
        s.dims[k] = (int32_t)std::floor((hi - s.origin[k]) / s.cell[k]) + 1;
    }
    return s;
}

static void plant_garbage(Mesh &m, unsigned seed) {
    std::mt19937 rng(seed);
    const int32_t bad[4] = {-1, (int32_t)m.nv(), 2147483647, std::numeric_limits<int32_t>::min()};
    for (int64_t f = 0; f < m.nf(); f++)
        if (rng() % 20 == 0) m.f[3 * f + rng() % 3] = bad[rng() % 4];
}

static void test_simplifications() {
    // a triangle: in one cell it vanishes, in three it survives with its bits
    Mesh tri{{0.25f, 0.25f, 0.25f, 0.75f, 0.25f, 0.5f, 0.25f, 0.75f, 0.5f}, {0, 1, 2}};
    {
        const Result r = check_case(tri, Space{{0, 0, 0}, {1, 1, 1}, {1, 1, 1}});
        EXPECT(r.v.empty() && r.f.empty() && r.cluster == std::vector<int32_t>({-1, -1, -1}));
        const Result k = check_case(tri, Space{{0, 0, 0}, {0.5, 0.5, 0.5}, {2, 2, 2}});
        EXPECT(k.f == std::vector<int32_t>({0, 1, 2}) && k.source == std::vector<int32_t>({0, 1, 2}));
        for (int i = 0; i < 9; i++) EXPECT(k.v[i] == bits_of(tri.v[i]));
    }
    Mesh tet{{0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2}};
    check_case(tet, Space{{-0.5, -0.5, -0.5}, {1, 1, 1}, {2, 2, 2}});
    check_case(tet, Space{{0, 0, 0}, {0.5, 0.5, 0.5}, {3, 3, 3}});
    check_case(tet, Space{{0, 0, 0}, {4, 4, 4}, {1, 1, 1}});
    // no faces at all
    check_case(Mesh{{1, 2, 3, 4, 5, 6}, {}}, Space{{0, 0, 0}, {1, 1, 1}, {8, 8, 8}});
    check_case(Mesh{{}, {}}, Space{{0, 0, 0}, {1, 1, 1}, {8, 8, 8}});
    for (int64_t nv : {4, 64, 65, 257})
        for (bool permuted : {false, true})
            for (double c : {0.25, 1.0, 3.5}) {
                const Mesh m = strip(nv, (unsigned)nv, permuted);
                check_case(m, around(m, c, c, c));
                check_case(m, around(m, c, 2.0 * c, 0.5 * c));
            }
    for (bool hub_last : {false, true}) {
        const Mesh m = star(50, 7, hub_last);
        check_case(m, around(m, 1.0, 1.0, 1.0));
        check_case(m, around(m, 3.0, 2.0, 5.0));
    }
    // 5000 vertices in ONE cell: the sums, the mean's exactness; everything collapses
    {
        Mesh m;
        std::mt19937 rng(11);
        std::uniform_real_distribution<float> in(0.001f, 0.999f);
        for (int i = 0; i < 5000; i++) {
            m.v.push_back(3.0f + in(rng));
            m.v.push_back(-2.0f + in(rng));
            m.v.push_back(7.0f + in(rng));
        }
        for (int i = 0; i + 2 < 5000; i++)
            for (int k = 0; k < 3; k++) m.f.push_back(i + k);
        const Result r = check_case(m, Space{{0, -5, 0}, {1, 1, 1}, {8, 8, 8}});
        EXPECT(r.f.empty() && r.v.empty());
        // two far vertices keep the big cluster in use
        Mesh n = m;
        for (float x : {0.5f, 0.5f, 0.5f, 6.5f, 0.5f, 0.5f}) n.v.push_back(x);
        for (int32_t i : {17, 5000, 5001}) n.f.push_back(i);
        const Result k = check_case(n, Space{{0, -5, 0}, {1, 1, 1}, {8, 8, 8}});
        EXPECT(k.f == std::vector<int32_t>({0, 1, 2}) && k.source == std::vector<int32_t>({0, 5000, 5001}));
    }
    for (unsigned seed : {1u, 2u, 3u}) {
        Mesh m = strip(257, 40 + seed, seed == 2);
        plant_garbage(m, seed);
        check_case(m, around(m, 1.0, 1.0, 1.0));
        check_case(m, around(m, 0.125, 0.125, 0.125));
    }
    // NaN and inf positions, far outside: singletons whose bits survive, faces between them too
    {
        Mesh m = strip(65, 5, false);
        const Space s = around(m, 1.0, 1.0, 1.0);
        const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
        m.v[3 * 10 + 1] = nan;
        m.v[3 * 11 + 0] = inf;
        m.v[3 * 12 + 2] = -inf;
        m.v[3 * 13 + 0] = 1e30f;
        m.v[3 * 40 + 0] = -1e30f;
        m.v[3 * 41 + 2] = std::numeric_limits<float>::max();
        const Result r = check_case(m, s);
        for (int32_t v : {10, 11, 12, 13}) {
            const int32_t o = r.cluster[v];
            EXPECT(o >= 0 && r.source[o] == v);
            if (o >= 0)
                for (int k = 0; k < 3; k++) EXPECT(r.v[3 * o + k] == bits_of(m.v[3 * v + k]));
        }
        Mesh all = m;
        for (auto &x : all.v) x = nan;
        const Result a = check_case(all, s);
        EXPECT((int64_t)a.source.size() == all.nv() && a.f == all.f);
    }
    // vertices on cell borders and on the grid's far faces: q == dims - 1 stays, q == dims does not
    {
        Mesh m;
        for (int i = 0; i <= 8; i++)
            for (int j = 0; j <= 4; j++) {
                m.v.push_back(0.5f * (float)i);
                m.v.push_back(0.75f * (float)j - 1.5f);
                m.v.push_back((i + j) % 2 ? 0.0f : 2.0f);
            }
        for (int i = 0; i < 8; i++)
            for (int j = 0; j < 4; j++) {
                const int32_t a = i * 5 + j, b = a + 5;
                for (int32_t x : {a, b, a + 1, a + 1, b, b + 1}) m.f.push_back(x);
            }
        check_case(m, Space{{0, -1.5, 0}, {0.5, 0.75, 2.0}, {8, 4, 1}});
        check_case(m, Space{{0, -1.5, 0}, {1.0, 1.5, 1.0}, {4, 2, 2}});
        check_case(m, Space{{0.5, -0.75, -2.0}, {1.5, 0.75, 2.0}, {2, 3, 2}});
        m.v[0] = -0.0f;
        m.v[3] = std::numeric_limits<float>::denorm_min();
        check_case(m, Space{{0, -1.5, 0}, {0.125, 0.125, 0.125}, {33, 25, 17}});
    }
}

int main() {
    test_verdict();
    test_layout();
    test_simplifications();
    std::printf("%d simplifications\n", cases);
    return finish("simplify");
}
