// quadric_args_main.cpp -- raynet_quadric_args.h on the host, under the address and
// undefined-behaviour sanitizers (tests/test_quadric_cpu.py builds and runs this program):
//   * the verdict of rn_mesh_place_quadric's arguments at every limit and one beyond it;
//   * the workspace layout;
//   * whole placements as the launcher's own sequence of phases, executed serially over the
//     header's functions in both orders of the threads, every buffer a heap block of exactly the
//     size the definition names, each result -- the eleven words of every output vertex, the bits
//     of positions_out and the two counts -- compared with what tests/quadric_truth.py gives for
//     the same mesh.  The meshes and the truth's results are quadric_expected.h, which the Python
//     test writes next to the program before it builds it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "raynet_quadric_args.h"
#include "host_main.h"
#include "quadric_expected.h"       // struct Case { ... }; static const Case CASES[]; N_CASES

using namespace rn_qd;

// ------------------------------------------------------------------------------ the verdict
static void test_verdict() {
    const double cell[3] = {1.0, 0.5, 2.0};
    alignas(8) char block[64];
    const void *vin = block, *fin = block + 8, *cl = block + 16, *pin = block + 24,
               *pout = block + 32, *counts = block + 40, *ws = block + 48;
    const double reg = 0.0009765625, move = 1.0;
    auto verdict = [&](int64_t nv, int64_t nf, int64_t nvo) {
        return place_args(true, nv, vin, nf, fin, cl, nvo, pin, cell, reg, move, pout, counts, ws);
    };
    const int64_t NV = ((int64_t)1 << 31) - 2, NF = (((int64_t)1 << 31) - 1) / 3;
    EXPECT(verdict(4, 2, 3) == LAUNCH);
    EXPECT(verdict(NV, NF, NV) == LAUNCH);
    EXPECT(verdict(NV + 1, 1, 1) == INVALID && verdict(4, NF + 1, 1) == INVALID);
    EXPECT(verdict(-1, 0, 0) == INVALID && verdict(4, -1, 1) == INVALID);
    EXPECT(verdict(4, 2, -1) == INVALID && verdict(4, 2, 5) == INVALID && verdict(4, 2, 4) == LAUNCH);
    EXPECT(verdict(4, 2, 0) == EMPTY && verdict(0, 0, 0) == EMPTY && verdict(0, 0, 1) == INVALID);
    EXPECT(place_args(false, 4, vin, 2, fin, cl, 3, pin, cell, reg, move, pout, counts, ws) == INVALID);
    // nvo == 0: whatever the device pointers, but not with bad scalars and not without counts
    EXPECT(place_args(true, 4, nullptr, 2, nullptr, nullptr, 0, nullptr, cell, reg, move, nullptr,
                      counts, nullptr) == EMPTY);
    EXPECT(place_args(true, 4, nullptr, 2, nullptr, nullptr, 0, nullptr, cell, reg, move, nullptr,
                      nullptr, nullptr) == INVALID);
    EXPECT(place_args(true, 4, nullptr, 2, nullptr, nullptr, 0, nullptr, cell, 2.0, move, nullptr,
                      counts, nullptr) == INVALID);
    EXPECT(place_args(true, 4, nullptr, 2, nullptr, nullptr, 0, nullptr, nullptr, reg, move, nullptr,
                      counts, nullptr) == INVALID);
    // the cell
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    for (int k = 0; k < 3; k++) {
        for (double bad : {0.0, -0.0, -1.0, inf, -inf, nan}) {
            double c[3] = {1.0, 0.5, 2.0};
            c[k] = bad;
            EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, c, reg, move, pout, counts, ws) == INVALID);
        }
        for (double good : {std::numeric_limits<double>::denorm_min(), 1e300,
                            std::numeric_limits<double>::max()}) {
            double c[3] = {1.0, 0.5, 2.0};
            c[k] = good;
            EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, c, reg, move, pout, counts, ws) == LAUNCH);
        }
    }
    // the regulariser: [2^-20, 1]; the clamp: > 0, inf included
    const double least = std::ldexp(1.0, -20);
    EXPECT(least == MIN_REGULARIZATION);
    for (double bad : {0.0, -1.0, std::nextafter(least, 0.0), std::nextafter(1.0, 2.0), inf, -inf, nan})
        EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, bad, move, pout, counts, ws) == INVALID);
    for (double good : {least, 0.0009765625, 1.0})
        EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, good, move, pout, counts, ws) == LAUNCH);
    for (double bad : {0.0, -0.0, -1.0, -inf, nan})
        EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, bad, pout, counts, ws) == INVALID);
    for (double good : {std::numeric_limits<double>::denorm_min(), 0.05, 1.0, 1e300, inf})
        EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, good, pout, counts, ws) == LAUNCH);
    // each pointer
    EXPECT(place_args(true, 4, nullptr, 2, fin, cl, 3, pin, cell, reg, move, pout, counts, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 2, nullptr, cl, 3, pin, cell, reg, move, pout, counts, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 2, fin, nullptr, 3, pin, cell, reg, move, pout, counts, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, nullptr, cell, reg, move, pout, counts, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, move, nullptr, counts, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, move, pout, nullptr, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, move, pout, counts, nullptr) == INVALID);
    EXPECT(place_args(true, 4, vin, 0, nullptr, cl, 3, pin, cell, reg, move, pout, counts, ws) == LAUNCH);
    // the alignment
    for (int off = 1; off < 8; off++)
        EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, move, pout, counts,
                          block + 48 + off) == INVALID);
    // the aliasings of positions_out
    for (const void *other : {vin, fin, cl, pin, ws})
        EXPECT(place_args(true, 4, vin, 2, fin, cl, 3, pin, cell, reg, move, other, counts, ws) == INVALID);
    EXPECT(place_args(true, 4, vin, 0, fin, cl, 3, pin, cell, reg, move, fin, counts, ws) == LAUNCH);
}

// ------------------------------------------------------------------------------- the layout
static void test_layout() {
    const int64_t NV = ((int64_t)1 << 31) - 2, NF = (((int64_t)1 << 31) - 1) / 3;
    EXPECT(WORDS == 11 && VERTEX_BYTES == 88 && COUNT == 10);
    EXPECT(workspace_bytes(0, 0, 0) == 0 && workspace_bytes(5, 3, 0) == 0);
    EXPECT(workspace_bytes(5, 3, 1) == 88 && workspace_bytes(257, 255, 100) == 8800);
    EXPECT(workspace_bytes(NV, NF, NV) == 88 * NV && workspace_bytes(NV, NF, NV) % 8 == 0);
    EXPECT(workspace_bytes(-1, 0, 0) == -1 && workspace_bytes(0, -1, 0) == -1);
    EXPECT(workspace_bytes(NV + 1, 0, 0) == -1 && workspace_bytes(1, NF + 1, 0) == -1);
    EXPECT(workspace_bytes(5, 3, -1) == -1 && workspace_bytes(5, 3, 6) == -1);
    for (int64_t k : {(int64_t)0, (int64_t)1, NV - 1})
        for (int word = 0; word < WORDS; word++) {
            EXPECT(word_index(k, word) == (size_t)(11 * k + word));
            EXPECT(8 * (int64_t)word_index(k, word) + 8 <= workspace_bytes(NV, NF, k + 1));
        }
    EXPECT(blocks(0, 256) == 1 && blocks(257, 256) == 2);
    // the rounding: to nearest, ties to even, of either sign, up to the bound of a term
    EXPECT(fixed(0.0) == 0 && fixed(-0.0) == 0 && fixed(1.0) == 1073741824 && fixed(-1.0) == -1073741824);
    const double unit = 1.0 / 1073741824.0;
    EXPECT(fixed(0.5 * unit) == 0 && fixed(1.5 * unit) == 2 && fixed(2.5 * unit) == 2);
    EXPECT(fixed(-0.5 * unit) == 0 && fixed(-1.5 * unit) == -2 && fixed(-2.5 * unit) == -2);
    EXPECT(fixed(0.75 * unit) == 1 && fixed(-0.75 * unit) == -1 && fixed(0.25 * unit) == 0);
    EXPECT(fixed(3.47) == (int64_t)std::rint(3.47 * 1073741824.0) && fixed(3.47) < ((int64_t)1 << 32));
    EXPECT(fixed(-3.47) == -fixed(3.47));
    EXPECT(is_finite(0.0) && is_finite(-LARGEST) && is_finite(LARGEST));
    EXPECT(!is_finite(std::nan("")) && !is_finite(std::numeric_limits<double>::infinity()) &&
           !is_finite(-std::numeric_limits<double>::infinity()));
    EXPECT(same_bits(1.5f, 1.5f) && !same_bits(0.0f, -0.0f) && same_bits(std::nanf(""), std::nanf("")));
}

// ------------------------------------------------------------------------- whole placements
static uint32_t bits_of(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return b;
}
static float float_of(uint32_t b) {
    float x;
    std::memcpy(&x, &b, 4);
    return x;
}

// the atomics policy of a serial run
struct SerialAtomics {
    void add_i64(int64_t *p, int64_t x) const { *p += x; }
    void count(int64_t *p) const { *p += 1; }
};

static void run_case(const Case &c, bool reversed) {
    const int64_t nv = c.nv, nf = c.nf, nvo = c.nvo;
    const uint32_t PRE = 0xFFC00777u;
    std::unique_ptr<float[]> vin(new float[3 * nv]), pin(new float[3 * nvo]), pout(new float[3 * nvo]);
    std::unique_ptr<int32_t[]> fin(new int32_t[3 * nf]), cl(new int32_t[nv]);
    std::unique_ptr<int64_t[]> counts(new int64_t[2]);
    for (int64_t i = 0; i < 3 * nv; i++) vin[i] = float_of(c.vertices[i]);
    for (int64_t i = 0; i < 3 * nvo; i++) pin[i] = float_of(c.positions[i]);
    for (int64_t i = 0; i < 3 * nvo; i++) pout[i] = float_of(PRE);
    for (int64_t i = 0; i < 3 * nf; i++) fin[i] = c.faces[i];
    for (int64_t i = 0; i < nv; i++) cl[i] = c.cluster[i];
    const int64_t bytes = workspace_bytes(nv, nf, nvo);
    EXPECT(bytes == 88 * nvo);
    std::unique_ptr<char[]> ws(new char[bytes > 0 ? bytes : 8]);
    std::memset(ws.get(), 0xA5, (size_t)(bytes > 0 ? bytes : 8));
    const Verdict verdict = place_args(true, nv, vin.get(), nf, fin.get(), cl.get(), nvo, pin.get(),
                                       c.cell, c.regularization, c.max_move, pout.get(),
                                       counts.get(), ws.get());
    counts[0] = counts[1] = 0;
    if (nvo == 0) {
        EXPECT(verdict == EMPTY);
        EXPECT(c.counts[0] == 0 && c.counts[1] == 0);
        return;
    }
    EXPECT(verdict == LAUNCH);
    const Solve s = solve_of(c.cell, c.regularization, c.max_move);
    EXPECT(s.L >= c.cell[0] && s.L >= c.cell[1] && s.L >= c.cell[2]);
    const Tables t = tables_of(nv, nf, nvo, ws.get());
    const SerialAtomics at{};
    for (int64_t i = 0; i < nvo; i++) clear(reversed ? nvo - 1 - i : i, t);
    for (int64_t i = 0; i < nv; i++) count_member(at, reversed ? nv - 1 - i : i, cl.get(), t);
    for (int64_t i = 0; i < nf; i++)
        add_face(at, reversed ? nf - 1 - i : i, vin.get(), fin.get(), cl.get(), pin.get(), s.L, t);
    for (int64_t i = 0; i < 11 * nvo; i++) {
        EXPECT(t.sums[i] == c.sums[i]);
        if (i % 11 != 10) EXPECT(t.sums[i] < ((int64_t)1 << 62) && t.sums[i] > -((int64_t)1 << 62));
    }
    for (int64_t i = 0; i < nvo; i++)
        solve_vertex(at, reversed ? nvo - 1 - i : i, pin.get(), s, t, pout.get(), counts.get());
    for (int64_t i = 0; i < 3 * nvo; i++) EXPECT(bits_of(pout[i]) == c.expected[i]);
    EXPECT(counts[0] == c.counts[0] && counts[1] == c.counts[1]);
    // the inputs are what they were
    for (int64_t i = 0; i < 3 * nv; i++) EXPECT(bits_of(vin[i]) == c.vertices[i]);
    for (int64_t i = 0; i < 3 * nvo; i++) EXPECT(bits_of(pin[i]) == c.positions[i]);
    for (int64_t i = 0; i < 3 * nf; i++) EXPECT(fin[i] == c.faces[i]);
    for (int64_t i = 0; i < nv; i++) EXPECT(cl[i] == c.cluster[i]);
}

int main() {
    test_verdict();
    test_layout();
    for (int i = 0; i < N_CASES; i++) {
        const int before = failures;
        run_case(CASES[i], false);
        run_case(CASES[i], true);
        if (failures != before) std::printf("case %s failed\n", CASES[i].name);
    }
    std::printf("%d placements\n", N_CASES);
    return finish("quadric");
}
