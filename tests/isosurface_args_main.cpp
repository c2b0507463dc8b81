// Stand-alone host program over raynet_amd/csrc/raynet_isosurface_args.h: the lattice sizes, the
// overflow bound, the workspace layout, the scan's level arithmetic, the refusals of
// rn_isosurface_count / rn_isosurface_emit and the rows the emit kernel may write, which hold no
// HIP and so run here without a GPU.  tests/test_isosurface_cpu.py builds it with
// -fsanitize=address,undefined and runs it; it exits 0 when every expectation holds and prints the
// first one that does not.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_isosurface_args.h"
#include "host_main.h"

using namespace rn_iso;

// what an entry returns for a verdict, before it launches anything
static int status(Verdict v) { return v == INVALID ? RN_ERR_INVALID : RN_OK; }

int main() {
    // ---- the lattice
    const Lattice open = lattice(12, 11, 10, 0), closed = lattice(12, 11, 10, 1);
    EXPECT(open.nx == 12 && open.ny == 11 && open.nz == 10 && open.points == 1320);
    EXPECT(open.cells == 11 * 10 * 9);
    EXPECT(closed.nx == 14 && closed.ny == 13 && closed.nz == 12 && closed.points == 2184);
    EXPECT(closed.cells == 13 * 12 * 11);
    EXPECT(lattice(1, 1, 1, 1).points == 27 && lattice(1, 1, 1, 1).cells == 8);
    EXPECT(lattice(1, 5, 5, 0).cells == 0 && lattice(5, 1, 5, 0).cells == 0 &&
           lattice(5, 5, 1, 0).cells == 0 && lattice(1, 1, 1, 0).cells == 0);
    EXPECT(max_vertices(lattice(1, 5, 5, 0)) == 0 && max_faces(lattice(1, 5, 5, 0)) == 0);
    EXPECT(max_vertices(closed) == 7 * 2184 && max_faces(closed) == 12 * 13 * 12 * 11);
    // ---- the overflow bound: 12 L < 2^31, in 64-bit arithmetic
    EXPECT(lattice_fits(lattice(128, 128, 128, 1)));
    EXPECT(lattice_fits(lattice(561, 561, 561, 1)));            // 563^3 = 178,453,547
    EXPECT(!lattice_fits(lattice(562, 562, 562, 1)));           // 564^3 = 179,406,144
    EXPECT(12 * lattice(561, 561, 561, 1).points < (1LL << 31));
    EXPECT(12 * lattice(562, 562, 562, 1).points >= (1LL << 31));
    EXPECT(!lattice_fits(lattice(1024, 1024, 1024, 0)));
    EXPECT(lattice(1 << 20, 1 << 20, 1 << 20, 0).points == (1LL << 60));     // 64-bit on the way
    EXPECT(!lattice_fits(lattice(1 << 20, 1 << 20, 1 << 20, 0)));
    EXPECT(!lattice_fits(lattice(0, 4, 4, 0)) && !lattice_fits(lattice(4, -1, 4, 0)));
    EXPECT(workspace_bytes(lattice(1024, 1024, 1024, 0)) == -1);
    // ---- the scan's levels
    EXPECT(scan_levels(1) == 1 && scan_levels(256) == 1 && scan_levels(257) == 2);
    EXPECT(scan_levels(65536) == 2 && scan_levels(65537) == 3);
    EXPECT(scan_levels(74088) == 3);                            // 42^3: 290 sums, then 2
    EXPECT(scan_scratch_words(256) == 0 && scan_scratch_words(257) == 2);
    EXPECT(scan_scratch_words(74088) == 290 + 2);
    EXPECT(scan_scratch_words(2184) == 9);
    EXPECT(scan_levels(178453547) == 4);
    // ---- the workspace: counts, scratch, total, masks, in this order and without overlap
    for (const Lattice &l : {closed, lattice(40, 40, 40, 1), lattice(1, 1, 1, 1),
                             lattice(3, 4, 5, 0)}) {
        EXPECT(ws_counts(l) == 0 && ws_scratch(l) == 8 * (size_t)l.points);
        EXPECT(ws_total(l) == ws_scratch(l) + 8 * (size_t)scan_scratch_words(l.points));
        EXPECT(ws_masks(l) == ws_total(l) + 8);
        EXPECT(workspace_bytes(l) >= (int64_t)(ws_masks(l) + l.points));
        EXPECT(workspace_bytes(l) % 8 == 0 && ws_total(l) % 8 == 0);
        // every byte the entries address lies in a heap block of exactly that size
        std::vector<unsigned char> ws((size_t)workspace_bytes(l), 0);
        ws[ws_counts(l) + 8 * (size_t)l.points - 1] = 1;
        ws[ws_total(l) + 7] = 2;
        ws[ws_masks(l) + (size_t)l.points - 1] = 3;
        EXPECT(ws[ws_masks(l) + (size_t)l.points - 1] == 3);
    }
    // ---- the refusals
    alignas(8) unsigned char buffer[16] = {0};
    const void *p = buffer;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float inf = std::numeric_limits<float>::infinity();
    EXPECT(count_args(true, closed, p, 0.5f, 1, p, p) == LAUNCH);
    EXPECT(count_args(true, open, p, 0.5f, 0, p, p) == LAUNCH);
    EXPECT(count_args(true, lattice(1, 5, 5, 0), p, 0.5f, 0, p, p) == EMPTY);
    EXPECT(status(count_args(false, closed, p, 0.5f, 1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, nullptr, 0.5f, 1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, 0.5f, 1, nullptr, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, 0.5f, 1, p, nullptr)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, 0.5f, 1, buffer + 4, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, 0.5f, 2, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, 0.5f, -1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, nan, 1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, inf, 0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, -inf, 0, p, p)) == RN_ERR_INVALID);
    // the padding's 0 must be outside: iso <= 0 only for an open lattice
    EXPECT(status(count_args(true, closed, p, 0.0f, 1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(count_args(true, closed, p, -0.25f, 1, p, p)) == RN_ERR_INVALID);
    EXPECT(count_args(true, open, p, 0.0f, 0, p, p) == LAUNCH);
    EXPECT(count_args(true, open, p, -0.25f, 0, p, p) == LAUNCH);
    EXPECT(status(count_args(true, lattice(562, 562, 562, 1), p, 0.5f, 1, p, p)) ==
           RN_ERR_INVALID);
    // emit: the totals of a count
    EXPECT(emit_args(true, closed, p, 0.5f, 1, p, 756, 1508, p, p) == LAUNCH);
    EXPECT(emit_args(true, closed, p, 0.5f, 1, p, 0, 0, nullptr, nullptr) == EMPTY);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 1, p, 756, 1508, nullptr, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 1, p, 756, 1508, p, nullptr)) ==
           RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 1, p, -1, 0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 1, p, 0, -1, p, p)) == RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 1, p, 7 * 2184 + 1, 4, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 1, p, 4, 12 * 1716 + 1, p, p)) ==
           RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, nullptr, 0.5f, 1, p, 0, 0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.0f, 1, p, 0, 0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(emit_args(true, closed, p, 0.5f, 3, p, 0, 0, p, p)) == RN_ERR_INVALID);
    EXPECT(status(emit_args(true, lattice(1, 5, 5, 0), p, 0.5f, 0, p, 1, 0, p, p)) ==
           RN_ERR_INVALID);

    // ---- the rows: heap arrays of exactly rows_extent(nv) floats and rows_extent(nf) ints take
    // every guarded write (the address sanitizer watches the ends), also when the offsets run
    // past the totals, as they would with a workspace that belongs to another count
    const int64_t nv = 197, nf = 391;
    EXPECT(rows_extent(0) == 0 && rows_extent(nv) == (size_t)(3 * nv));
    std::vector<float> vertices(rows_extent(nv), -7.0f);
    std::vector<int32_t> faces(rows_extent(nf), -7);
    for (int64_t row = -3; row < nv + 50; row++)
        if (row_in(row, nv))
            for (int c = 0; c < 3; c++) vertices[row_index(row, c)] = (float)row;
    for (int64_t row = -3; row < nf + 50; row++)
        if (row_in(row, nf))
            for (int c = 0; c < 3; c++) faces[row_index(row, c)] = (int32_t)row;
    EXPECT(vertices[0] == 0.0f && vertices[rows_extent(nv) - 1] == (float)(nv - 1));
    EXPECT(faces[0] == 0 && faces[rows_extent(nf) - 1] == (int32_t)(nf - 1));
    EXPECT(!row_in(nv, nv) && !row_in(-1, nv) && !row_in(0, 0));
    // no 32-bit overflow: the last entry of the largest outputs
    EXPECT(row_index(0x7ffffffeLL, 2) == 3 * (size_t)0x7ffffffeULL + 2);
    // ---- the count words: two 32-bit halves, no carry between them up to the bound
    const uint64_t w = pack_counts(7, 12);
    EXPECT(count_vertices(w) == 7 && count_faces(w) == 12);
    const uint64_t sum = (uint64_t)178453547 * w;
    EXPECT(count_vertices(sum) == 7LL * 178453547 && count_faces(sum) == 12LL * 178453547);
    EXPECT(count_faces(sum) < (1LL << 31));
    return finish("isosurface");
}
