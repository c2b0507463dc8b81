// Stand-alone host program over raynet_amd/csrc/raynet_render_args.h: every verdict of
// rn_mesh_render's argument check at and beside each limit, against a second statement of the
// rules written here from the entry's contract (include/raynet_hip.h), and the two lane mappings:
// each names every pixel of every view exactly once and nothing else, so that no lane addresses an
// output out of bounds.  The header holds no HIP, so all of it runs without a GPU.
// tests/test_render_cpu.py builds it with -fsanitize=address,undefined and runs it; it exits 0
// when every expectation holds and prints the first one that does not.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/raynet_hip.h"
#include "raynet_render_args.h"
#include "host_main.h"

using namespace rn_render;

struct Args {
    bool ctx = true;
    int64_t nv = 4, nf = 2;
    int32_t C = 3, V = 2, H = 5, W = 7;
    // 0: null.  nodes leaves vertices faces colors normals cameras face depth bary color normal
    bool p[12] = {true, true, true, true, true, true, true, true, true, true, true, true};
};
enum { NODES, LEAVES, VERTICES, FACES, COLORS, NORMALS, CAMERAS, FACE, DEPTH, BARY, COLOR, NORMAL };

static unsigned char block[12];
static const void *ptr(const Args &a, int k) { return a.p[k] ? block + k : nullptr; }

static Verdict verdict(const Args &a) {
    return render_args(a.ctx, ptr(a, NODES), ptr(a, LEAVES), a.nv, ptr(a, VERTICES), a.nf,
                       ptr(a, FACES), ptr(a, COLORS), a.C, ptr(a, NORMALS), a.V, ptr(a, CAMERAS),
                       a.H, a.W, ptr(a, FACE), ptr(a, DEPTH), ptr(a, BARY), ptr(a, COLOR),
                       ptr(a, NORMAL));
}

// the contract, in 128-bit arithmetic so that nothing here can overflow
static Verdict by_contract(const Args &a) {
    typedef __int128 wide;
    const wide limit = ((wide)1 << 31) - 1;
    if (!a.ctx) return INVALID;
    if (a.nv < 0 || a.nf < 0 || a.V < 0 || a.H < 0 || a.W < 0) return INVALID;
    if (a.V > 4096) return INVALID;
    const wide n = (wide)a.V * a.H * a.W;
    if (n > limit) return INVALID;
    if (a.p[COLORS] && (a.C < 1 || a.C > 4)) return INVALID;
    if (a.p[COLORS] && n * a.C > limit) return INVALID;
    if ((wide)a.nv > limit - 1 || (wide)a.nf * 3 > limit) return INVALID;      // sizes_ok
    if (a.nf < 1) return INVALID;
    if (a.V == 0 || (wide)a.H * a.W == 0) return EMPTY;
    for (int k : {NODES, LEAVES, VERTICES, FACES, CAMERAS, FACE, DEPTH, BARY})
        if (!a.p[k]) return INVALID;
    if (a.p[COLORS] != a.p[COLOR] || a.p[NORMALS] != a.p[NORMAL]) return INVALID;
    return LAUNCH;
}

static int checked = 0;
static void check(const Args &a, int line) {
    checked++;
    if (verdict(a) != by_contract(a)) {
        std::printf("line %d: verdict %d, the contract says %d (nv %lld nf %lld C %d V %d H %d W %d)\n",
                    line, (int)verdict(a), (int)by_contract(a), (long long)a.nv, (long long)a.nf,
                    a.C, a.V, a.H, a.W);
        failures++;
    }
}
#define CHECK(a) check(a, __LINE__)

// every pixel of every view once, nothing else; lanes beyond the mapping's count name none
static void mapping(int32_t V, int32_t H, int32_t W) {
    const int64_t n = (int64_t)V * H * W;
    for (int tiled = 0; tiled < 2; tiled++) {
        std::vector<int> seen((size_t)n, 0);
        const int64_t lanes = tiled ? lanes_tiled(V, H, W) : lanes_rows(V, H, W);
        const int64_t upto = blocks(lanes, 128) * 128 + 130;
        int64_t named = 0;
        for (int64_t lane = -2; lane < upto; lane++) {
            const Pixel p = tiled ? (lane < 0 ? pixel_of_tile(-1, 0, V, H, W)
                                              : pixel_of_tile(lane / TILE_PIXELS,
                                                              (int)(lane % TILE_PIXELS), V, H, W))
                                  : pixel_of_row(lane, V, H, W);
            if (p.view < 0) continue;
            EXPECT(lane >= 0 && lane < lanes);
            EXPECT(p.view < V && p.row >= 0 && p.row < H && p.column >= 0 && p.column < W);
            const size_t at = pixel_index(p, H, W);
            EXPECT(at < (size_t)n);
            if (at < (size_t)n) seen[at]++;
            named++;
        }
        EXPECT(named == n);
        for (int64_t i = 0; i < n; i++)
            if (seen[(size_t)i] != 1) {
                std::printf("V %d H %d W %d, %s: pixel %lld named %d times\n", V, H, W,
                            tiled ? "tiles" : "rows", (long long)i, seen[(size_t)i]);
                failures++;
                break;
            }
    }
}

int main() {
    const int32_t i32max = std::numeric_limits<int32_t>::max(), i32min = std::numeric_limits<int32_t>::min();
    const int64_t i64max = std::numeric_limits<int64_t>::max(), i64min = std::numeric_limits<int64_t>::min();
    const int64_t max_nv = ((int64_t)1 << 31) - 2, max_nf = (((int64_t)1 << 31) - 1) / 3;
    Args good;
    EXPECT(verdict(good) == LAUNCH && by_contract(good) == LAUNCH);
    EXPECT(RN_ERR_INVALID == -1 && RN_OK == 0);

    // ---- the scalars, each at and beside its limits, alone and with no pixel to render
    for (int empty = 0; empty < 3; empty++) {
        Args base;
        if (empty == 1) base.V = 0;
        if (empty == 2) base.W = 0;
        for (int64_t nv : {i64min, (int64_t)-1, (int64_t)0, (int64_t)1, max_nv - 1, max_nv, max_nv + 1, i64max}) {
            Args a = base;
            a.nv = nv;
            CHECK(a);
        }
        for (int64_t nf : {i64min, (int64_t)-1, (int64_t)0, (int64_t)1, max_nf - 1, max_nf, max_nf + 1, i64max}) {
            Args a = base;
            a.nf = nf;
            CHECK(a);
        }
        for (int32_t C : {i32min, -1, 0, 1, 2, 3, 4, 5, i32max})
            for (int colours = 0; colours < 2; colours++) {
                Args a = base;
                a.C = C;
                a.p[COLORS] = a.p[COLOR] = colours != 0;
                CHECK(a);
            }
        for (int32_t V : {i32min, -1, 0, 1, 4095, 4096, 4097, i32max}) {
            Args a = base;
            a.V = V;
            CHECK(a);
        }
        for (int32_t H : {i32min, -1, 0, 1, i32max})
            for (int32_t W : {i32min, -1, 0, 1, i32max}) {
                Args a = base;
                a.H = H;
                a.W = W;
                CHECK(a);
                a.V = empty == 1 ? 0 : 1;
                CHECK(a);
            }
    }
    // ---- V H W and V H W C around 2^31 - 1
    {
        Args a;
        a.V = 1; a.H = 1; a.W = i32max; a.p[COLORS] = a.p[COLOR] = false;
        CHECK(a);
        EXPECT(verdict(a) == LAUNCH);
        a.p[COLORS] = a.p[COLOR] = true; a.C = 1;
        CHECK(a);
        EXPECT(verdict(a) == LAUNCH);
        a.C = 2;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        a.p[COLORS] = a.p[COLOR] = false;
        a.V = 2;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        a.V = 1; a.H = 2;
        CHECK(a);
        // 2^16 x 2^15 = 2^31: one too many; one row less fits
        a.H = 1 << 16; a.W = 1 << 15;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        a.H = (1 << 16) - 1;
        CHECK(a);
        EXPECT(verdict(a) == LAUNCH);
        // 4096 views of 2^19 - 1 pixels fit, of 2^19 not; with colours the channels count
        a.V = 4096; a.H = 1; a.W = (1 << 19) - 1;
        CHECK(a);
        EXPECT(verdict(a) == LAUNCH);
        a.W = 1 << 19;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        a.p[COLORS] = a.p[COLOR] = true;
        for (int32_t C : {1, 2, 3, 4}) {
            a.C = C;
            a.W = (i32max / 4096) / C;
            CHECK(a);
            EXPECT(verdict(a) == LAUNCH);
            a.W += 1;
            CHECK(a);
        }
        a.V = 4096; a.H = i32max; a.W = i32max; a.C = 4;       // the largest product there is
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        a.V = 0;                                               // no view: no pixel
        CHECK(a);
        EXPECT(verdict(a) == EMPTY);
        EXPECT(pixels(4096, i32max, i32max) == -1 && pixels(0, i32max, i32max) == 0);
        EXPECT(pixels(1, 1, i32max) == i32max && pixels(3, 7, 9) == 189 && pixels(1, 0, i32max) == 0);
    }
    // ---- the pointers: each alone, every pair of an attribute and its image, with and without
    // pixels to render
    for (int empty = 0; empty < 3; empty++)
        for (int mask = 0; mask < 16; mask++)
            for (int null_at = -1; null_at < 12; null_at++) {
                Args a;
                if (empty == 1) a.V = 0;
                if (empty == 2) a.H = 0;
                a.p[COLORS] = mask & 1; a.p[COLOR] = (mask >> 1) & 1;
                a.p[NORMALS] = (mask >> 2) & 1; a.p[NORMAL] = (mask >> 3) & 1;
                if (null_at >= 0) a.p[null_at] = false;
                CHECK(a);
            }
    {
        Args a;
        a.ctx = false;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        a.V = 0;
        CHECK(a);
        EXPECT(verdict(a) == INVALID);
        Args none;                          // nothing to do: whatever the pointers
        none.V = 0;
        for (bool &p : none.p) p = false;
        EXPECT(verdict(none) == EMPTY);
        none.V = 3; none.H = 0;
        EXPECT(verdict(none) == EMPTY);
        none.H = 4; none.W = 0;
        EXPECT(verdict(none) == EMPTY);
        none.nf = 0;                        // ... but not whatever the sizes
        EXPECT(verdict(none) == INVALID);
    }
    EXPECT(checked > 900);

    // ---- the mappings
    for (int32_t V : {1, 2, 3})
        for (int32_t H : {1, 7, 8, 9, 16, 20})
            for (int32_t W : {1, 7, 8, 9, 17, 30}) mapping(V, H, W);
    mapping(5, 1, 129);
    mapping(1, 130, 1);
    EXPECT(tiles_across(0) == 0 && tiles_across(1) == 1 && tiles_across(8) == 1 && tiles_across(9) == 2);
    EXPECT(tiles_across(i32max) == ((int64_t)1 << 28));
    EXPECT(lanes_tiled(3, 7, 9) == 3 * 2 * 64 && lanes_rows(3, 7, 9) == 189);
    EXPECT(lanes_tiled(1, 1, i32max) == ((int64_t)1 << 34) && blocks(lanes_tiled(1, 1, i32max), 128) < i32max);
    EXPECT(lanes_tiled(4096, 1, (1 << 19) - 1) == (int64_t)4096 * (1 << 16) * 64);
    EXPECT(blocks(lanes_tiled(4096, 1, (1 << 19) - 1), 128) < i32max);
    EXPECT(blocks(0, 128) == 0 && blocks(1, 128) == 1 && blocks(128, 128) == 1 && blocks(129, 128) == 2);
    EXPECT(pixel_of_tile(0, 0, 0, 8, 8).view == -1 && pixel_of_row(0, 0, 8, 8).view == -1);
    EXPECT(pixel_of_tile(0, 0, 1, 0, 8).view == -1 && pixel_of_row(0, 1, 8, 0).view == -1);
    {
        const Pixel p = pixel_of_tile(3, 63, 2, 7, 9);         // view 1, the tile right of the first
        EXPECT(p.view == -1);                                  // row 7 of 7: over the lower edge
        const Pixel q = pixel_of_tile(3, 8, 2, 7, 9);
        EXPECT(q.view == 1 && q.row == 1 && q.column == 8);
        EXPECT(pixel_index(q, 7, 9) == 63 + 9 + 8);
        const Pixel last{4095, 0, (1 << 19) - 2};
        EXPECT(pixel_index(last, 1, (1 << 19) - 1) == (size_t)4096 * ((1 << 19) - 1) - 1);
    }
    return finish("render");
}
