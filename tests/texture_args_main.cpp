// Stand-alone host program over raynet_amd/csrc/raynet_texture_args.h: every verdict of
// rn_texture_bake's and rn_texture_sample's argument checks at and beside each limit, against a
// second statement of the rules written here from the entries' contract (include/raynet_hip.h);
// the owner of every texel and the chart coordinates against a second, table-driven implementation
// (a table of owners painted cell by cell and row by row) for all nf <= 40, T <= 6 and several
// widths, every index in bounds; and the two lane mappings: each names every texel exactly once
// and nothing else.  The header holds no HIP, so all of it runs without a GPU.
// tests/test_texture_cpu.py builds it with -fsanitize=address,undefined and runs it; it exits 0
// when every expectation holds and prints the first one that does not.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_texture_args.h"
#include "host_main.h"

using namespace rn_tex;

static unsigned char block[16];
static const void *ptr(bool have, int k) { return have ? block + k : nullptr; }

// ------------------------------------------------------------------------------ the bake's check
struct Bake {
    bool ctx = true;
    int64_t nv = 5, nf = 4;
    int32_t T = 4, Cw = 2, V = 2, H = 5, W = 7, C = 3, mode = 0;
    double tol = 0.1, min_cos = 0.0, border = 0.0;
    // vertices faces cameras images texture weight views
    bool p[7] = {true, true, true, true, true, true, true};
};
enum { VERTICES, FACES, CAMERAS, IMAGES, TEXTURE, WEIGHT, VIEWS };

static Verdict verdict(const Bake &a) {
    return bake_args(a.ctx, a.nv, ptr(a.p[VERTICES], 0), a.nf, ptr(a.p[FACES], 1), a.T, a.Cw, a.V,
                     ptr(a.p[CAMERAS], 2), a.H, a.W, a.C, ptr(a.p[IMAGES], 3), a.tol, a.min_cos,
                     a.border, a.mode, ptr(a.p[TEXTURE], 4), ptr(a.p[WEIGHT], 5),
                     ptr(a.p[VIEWS], 6));
}

typedef __int128 wide;
static const wide LIMIT = ((wide)1 << 31) - 1;

// the atlas of the contract, in 128-bit arithmetic: false where it cannot be addressed
static bool atlas_fits(int64_t nf, int32_t T, int32_t Cw, int32_t C) {
    const wide cells = ((wide)nf + 1) / 2, S = (wide)T + 5;
    if (cells == 0) return true;
    const wide rows = (cells + Cw - 1) / Cw, Wt = Cw * S, Ht = rows * S;
    return Wt <= 16384 && Ht <= 16384 && Wt * Ht * C <= LIMIT;
}

static Verdict by_contract(const Bake &a) {
    if (!a.ctx) return INVALID;
    if (a.nv < 0 || a.nf < 0 || (wide)a.nv > LIMIT - 1 || (wide)a.nf * 3 > LIMIT) return INVALID;
    if (a.T < 1 || a.T > 1024 || a.Cw < 1 || a.Cw > 16384) return INVALID;
    if (a.V < 0 || a.V > 32 || a.C < 1 || a.C > 4 || a.H < 1 || a.W < 1) return INVALID;
    if (!(a.tol >= 0.0) || std::isinf(a.tol)) return INVALID;
    if (!(a.min_cos >= 0.0 && a.min_cos < 1.0)) return INVALID;
    if (!(a.border >= 0.0) || std::isinf(a.border)) return INVALID;
    if (a.mode != 0 && a.mode != 1) return INVALID;
    if (!atlas_fits(a.nf, a.T, a.Cw, a.C)) return INVALID;
    if (a.nf == 0) return EMPTY;
    for (int k : {VERTICES, FACES, TEXTURE, WEIGHT, VIEWS})
        if (!a.p[k]) return INVALID;
    if (a.V > 0 && (!a.p[CAMERAS] || !a.p[IMAGES])) return INVALID;
    return LAUNCH;
}

static int checked = 0;
static void check(const Bake &a, int line) {
    checked++;
    if (verdict(a) != by_contract(a)) {
        std::printf("line %d: bake verdict %d, the contract says %d (nv %lld nf %lld T %d Cw %d V %d "
                    "H %d W %d C %d mode %d)\n", line, (int)verdict(a), (int)by_contract(a),
                    (long long)a.nv, (long long)a.nf, a.T, a.Cw, a.V, a.H, a.W, a.C, a.mode);
        failures++;
    }
}

// ------------------------------------------------------------------------------ the lookup's
struct Sample {
    bool ctx = true;
    int64_t n = 10, nf = 4;
    int32_t T = 4, Cw = 2, C = 3, bilinear = 1;
    bool p[4] = {true, true, true, true};       // face bary texture color
};
enum { FACE, BARY, ATLAS, COLOR };

static Verdict verdict(const Sample &a) {
    return sample_args(a.ctx, a.n, ptr(a.p[FACE], 0), ptr(a.p[BARY], 1), a.nf, a.T, a.Cw, a.C,
                       ptr(a.p[ATLAS], 2), a.bilinear, ptr(a.p[COLOR], 3));
}

static Verdict by_contract(const Sample &a) {
    if (!a.ctx) return INVALID;
    if (a.n < 0 || a.nf < 0 || (wide)a.nf * 3 > LIMIT) return INVALID;
    if (a.T < 1 || a.T > 1024 || a.Cw < 1 || a.Cw > 16384) return INVALID;
    if (a.C < 1 || a.C > 4 || (a.bilinear != 0 && a.bilinear != 1)) return INVALID;
    if ((wide)a.n * a.C > LIMIT) return INVALID;
    if (!atlas_fits(a.nf, a.T, a.Cw, a.C)) return INVALID;
    if (a.n == 0) return EMPTY;
    if (!a.p[FACE] || !a.p[BARY] || !a.p[COLOR]) return INVALID;
    if (a.nf > 0 && !a.p[ATLAS]) return INVALID;
    return LAUNCH;
}

static void check(const Sample &a, int line) {
    checked++;
    if (verdict(a) != by_contract(a)) {
        std::printf("line %d: sample verdict %d, the contract says %d (n %lld nf %lld T %d Cw %d C %d "
                    "bilinear %d)\n", line, (int)verdict(a), (int)by_contract(a), (long long)a.n,
                    (long long)a.nf, a.T, a.Cw, a.C, a.bilinear);
        failures++;
    }
}
#define CHECK(a) check(a, __LINE__)

// ------------------------------------------------------------------------------ the layout
// The second implementation: a table of Ht x Wt owners painted cell by cell, row by row: row j of
// a cell gives the cell's lower face its first T + 4 - j texels (none from row T + 4 on) and the
// upper face the rest.
static void layout(int64_t nf, int32_t T, int32_t Cw) {
    const Layout L = layout_of(nf, T, Cw);
    const int32_t S = T + 5;
    EXPECT(L.S == S && L.cells == (nf + 1) / 2 && L.Wt == (int64_t)Cw * S && L.Ht == L.rows * S);
    EXPECT(L.rows * Cw >= L.cells && (L.cells == 0 || (L.rows - 1) * Cw < L.cells));
    const size_t texels = (size_t)(L.Wt * L.Ht);
    std::vector<int64_t> table(texels, -1);
    auto table_p = exact(table);
    for (int64_t cell = 0; cell < L.rows * Cw; cell++) {
        const int64_t x = cell % Cw * S, y = cell / Cw * S;
        for (int32_t j = 0; j < S; j++)
            for (int32_t i = 0; i < S; i++) {
                const bool first = i < T + 4 - j;
                const int64_t f = 2 * cell + (first ? 0 : 1);
                const size_t at = (size_t)((y + j) * L.Wt + (x + i));
                EXPECT(at < texels);
                if (at < texels) table_p[at] = f < nf ? f : -1;
            }
    }
    std::vector<int> owned((size_t)nf + 1, 0);
    for (int64_t ty = 0; ty < L.Ht; ty++)
        for (int64_t tx = 0; tx < L.Wt; tx++) {
            const Owner o = owner_of(tx, ty, nf, T, Cw);
            const size_t at = texel_index(tx, ty, L.Wt);
            EXPECT(at < texels && o.face == table_p[at]);
            EXPECT(o.i >= 0 && o.i < S && o.j >= 0 && o.j < S && o.face >= -1 && o.face < nf);
            EXPECT(o.lower == (o.i + o.j <= T + 3));
            if (o.face >= 0) {
                owned[(size_t)o.face]++;
                EXPECT(is_lower(o.face) == o.lower && cell_column(o.face, Cw) == tx / S &&
                       cell_row(o.face, Cw) == ty / S);
                // the texel's raw barycentrics lead back to the texel
                const double u = raw_coordinate(o.lower, o.i, T), v = raw_coordinate(o.lower, o.j, T);
                EXPECT(std::fabs(chart_coordinate(o.lower, u, T) - o.i) < 1e-12);
                EXPECT(std::fabs(chart_coordinate(o.lower, v, T) - o.j) < 1e-12);
            }
        }
    const int half = (T + 4) * (T + 5) / 2;
    for (int64_t f = 0; f < nf; f++) {
        EXPECT(owned[(size_t)f] == (f % 2 == 0 ? half : S * S - half));
        // the corners, and the footprint of a bilinear lookup along the chart's rim and inside it
        const bool lower = is_lower(f);
        const int64_t x = cell_column(f, Cw) * S, y = cell_row(f, Cw) * S;
        EXPECT(chart_coordinate(lower, 0.0, T) == (lower ? 1 : T + 3));
        EXPECT(chart_coordinate(lower, 1.0, T) == (lower ? T + 1 : 3));
        const int steps = 2 * T + 3;
        for (int a = 0; a <= steps; a++)
            for (int b = 0; a + b <= steps; b++) {
                const double u = (double)a / steps, v = (double)b / steps;
                const double cx = chart_coordinate(lower, u, T), cy = chart_coordinate(lower, v, T);
                EXPECT(cx >= 1 && cx <= T + 3 && cy >= 1 && cy <= T + 3);
                const int64_t x0 = x + (int64_t)std::floor(cx), y0 = y + (int64_t)std::floor(cy);
                const double fx = cx - std::floor(cx), fy = cy - std::floor(cy);
                for (int dy = 0; dy < 2; dy++)
                    for (int dx = 0; dx < 2; dx++) {
                        if ((dx && fx == 0.0) || (dy && fy == 0.0)) continue;   // weight 0
                        const int64_t tx = x0 + dx, ty = y0 + dy;
                        EXPECT(tx >= 0 && tx < L.Wt && ty >= 0 && ty < L.Ht);
                        if (tx >= 0 && tx < L.Wt && ty >= 0 && ty < L.Ht)
                            EXPECT(table_p[texel_index(tx, ty, L.Wt)] == f);
                    }
                const int64_t xr = x + (int64_t)std::nearbyint(cx), yr = y + (int64_t)std::nearbyint(cy);
                EXPECT(xr >= 0 && xr < L.Wt && yr >= 0 && yr < L.Ht);
                if (xr >= 0 && xr < L.Wt && yr >= 0 && yr < L.Ht)
                    EXPECT(table_p[texel_index(xr, yr, L.Wt)] == f);
            }
    }
    // ---- the mappings: every texel once, nothing else
    for (int tiled = 0; tiled < 2; tiled++) {
        std::vector<int> seen(texels, 0);
        const int64_t lanes = tiled ? lanes_tiled(L.Wt, L.Ht) : lanes_rows(L.Wt, L.Ht);
        const int64_t upto = blocks(lanes, 256) * 256 + 70;
        int64_t named = 0;
        for (int64_t lane = -2; lane < upto; lane++) {
            const Texel t = tiled ? (lane < 0 ? texel_of_tile(-1, 0, L.Wt, L.Ht)
                                              : texel_of_tile(lane / TILE_TEXELS,
                                                              (int)(lane % TILE_TEXELS), L.Wt, L.Ht))
                                  : texel_of_row(lane, L.Wt, L.Ht);
            if (t.x < 0) continue;
            EXPECT(lane >= 0 && lane < lanes && t.x < L.Wt && t.y >= 0 && t.y < L.Ht);
            const size_t at = texel_index(t.x, t.y, L.Wt);
            EXPECT(at < texels);
            if (at < texels) seen[at]++;
            named++;
        }
        EXPECT(named == (int64_t)texels);
        for (int s : seen) EXPECT(s == 1);
    }
}

int main() {
    const int32_t i32max = std::numeric_limits<int32_t>::max();
    const int64_t i64max = std::numeric_limits<int64_t>::max();
    const double inf = std::numeric_limits<double>::infinity(), not_a_number = std::nan("");

    // ---- rn_texture_bake: each scalar at and beside its limits
    for (int64_t nv : {(int64_t)-1, (int64_t)0, (int64_t)5, (int64_t)i32max - 1, (int64_t)i32max, i64max})
        for (int64_t nf : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)4, (int64_t)i32max / 3,
                           (int64_t)i32max / 3 + 1, i64max}) {
            Bake a;
            a.nv = nv; a.nf = nf;
            CHECK(a);
            a.Cw = 16384; a.T = 1;
            CHECK(a);
        }
    for (int32_t T : {i32max, -i32max - 1, -1, 0, 1, 2, 1024, 1025})
        for (int32_t Cw : {i32max, -i32max - 1, -1, 0, 1, 2, 16, 17, 16384, 16385}) {
            Bake a;
            a.T = T; a.Cw = Cw;
            CHECK(a);
            a.nf = 2 * 16 * 16;         // 16 x 16 cells at Cw = 16: 1029 texels a cell at T = 1024
            CHECK(a);
            a.nf = 0;
            CHECK(a);
        }
    // the extents at their limit: S = 8, 2048 cells a row, 2048 rows
    for (int32_t Cw : {2047, 2048, 2049})
        for (int64_t rows : {2047, 2048, 2049})
            for (int64_t last : {0, 1, 2}) {
                Bake a;
                a.T = 3; a.Cw = Cw; a.C = 4;
                a.nf = 2 * ((rows - 1) * Cw) + last;
                a.nv = 3;
                CHECK(a);
            }
    for (int32_t V : {-1, 0, 1, 32, 33, i32max})
        for (int32_t C : {-1, 0, 1, 4, 5})
            for (int32_t H : {-1, 0, 1})
                for (int32_t mode : {-1, 0, 1, 2}) {
                    Bake a;
                    a.V = V; a.C = C; a.H = H; a.mode = mode;
                    CHECK(a);
                    a.W = 0;
                    CHECK(a);
                    a.W = 3; a.nf = 0;
                    CHECK(a);
                }
    for (double x : {-1.0, -0.0, 0.0, 0.5, 1.0, 2.0, inf, -inf, not_a_number}) {
        Bake a;
        a.tol = x;
        CHECK(a);
        a = Bake();
        a.min_cos = x;
        CHECK(a);
        a = Bake();
        a.border = x;
        CHECK(a);
    }
    for (int V : {0, 2})
        for (int nf : {0, 4})
            for (int mask = 0; mask < 128; mask++) {
                Bake a;
                a.V = V; a.nf = nf;
                for (int k = 0; k < 7; k++) a.p[k] = (mask >> k) & 1;
                CHECK(a);
            }
    {
        Bake a;
        a.ctx = false;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        Bake none;
        none.nf = 0;
        for (bool &p : none.p) p = false;
        EXPECT(verdict(none) == EMPTY);
        none.T = 0;                         // ... but not whatever the scalars
        EXPECT(verdict(none) == INVALID);
        EXPECT(verdict(Bake()) == LAUNCH);
    }

    // ---- rn_texture_sample
    for (int64_t n : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)i32max / 4, (int64_t)i32max / 4 + 1,
                      (int64_t)i32max / 3, (int64_t)i32max / 3 + 1, (int64_t)i32max, i64max})
        for (int32_t C : {-1, 0, 1, 3, 4, 5})
            for (int64_t nf : {(int64_t)-1, (int64_t)0, (int64_t)4, (int64_t)i32max / 3 + 1}) {
                Sample a;
                a.n = n; a.C = C; a.nf = nf;
                CHECK(a);
            }
    for (int32_t T : {-1, 0, 1, 1024, 1025})
        for (int32_t Cw : {-1, 0, 1, 16, 17, 16384, 16385})
            for (int32_t bilinear : {-1, 0, 1, 2}) {
                Sample a;
                a.T = T; a.Cw = Cw; a.bilinear = bilinear;
                CHECK(a);
                a.nf = 2 * 16 * 16;
                CHECK(a);
            }
    for (int n : {0, 10})
        for (int nf : {0, 4})
            for (int mask = 0; mask < 16; mask++) {
                Sample a;
                a.n = n; a.nf = nf;
                for (int k = 0; k < 4; k++) a.p[k] = (mask >> k) & 1;
                CHECK(a);
            }
    {
        Sample a;
        a.ctx = false;
        CHECK(a);
        EXPECT(verdict(a) == INVALID && verdict(Sample()) == LAUNCH);
    }
    EXPECT(checked > 1500);

    // ---- the layout, the owners, the footprints and the mappings
    for (int64_t nf = 0; nf <= 40; nf++)
        for (int32_t T = 1; T <= 6; T++)
            for (int32_t Cw : {1, 2, 3, 8, 21}) layout(nf, T, Cw);
    {
        // the largest atlas: nothing overflows, the last texel is the last entry
        const int64_t nf = 2 * (int64_t)2048 * 2048;
        const Layout L = layout_of(nf, 3, 2048);
        EXPECT(L.Wt == 16384 && L.Ht == 16384 && extents_ok(L));
        const Owner o = owner_of(L.Wt - 1, L.Ht - 1, nf, 3, 2048);
        EXPECT(o.face == nf - 1 && !o.lower && o.i == 7 && o.j == 7);
        EXPECT(texel_index(L.Wt - 1, L.Ht - 1, L.Wt) == (size_t)16384 * 16384 - 1);
        EXPECT(lanes_tiled(L.Wt, L.Ht) == lanes_rows(L.Wt, L.Ht));
        EXPECT(blocks(lanes_tiled(L.Wt, L.Ht), 256) == (1 << 20));
        const Layout M = layout_of((int64_t)i32max / 3, 1024, 1);
        EXPECT(!extents_ok(M) && M.Ht > 0);
        EXPECT(texel_of_tile(0, 0, 0, 8).x == -1 && texel_of_row(0, 0, 8).x == -1);
        EXPECT(texel_of_tile(0, 0, 8, 0).x == -1 && texel_of_row(0, 8, 0).x == -1);
        EXPECT(tiles_across(0) == 0 && tiles_across(8) == 1 && tiles_across(9) == 2);
    }
    return finish("texture");
}
