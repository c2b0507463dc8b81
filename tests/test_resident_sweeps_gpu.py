"""The RESIDENT BP and depth sweeps -- k_bp<NCH, true, false, STEADY>, k_depth<NCH, true, false,
STEADY> and k_depth_stats of csrc/raynet_mrf.inl: packed voxel words, 4x4x4-bricked accumulators,
columns already clipped -- per launch and per flag against the float64 truths of
tests/mrf_bwd_truth.py, on the fixtures of tests/resident_truth.py (whose conditions
tests/test_resident_truth.py asserts on the CPU).  Needs a real MI355X: `-m gpu`.

Routes of the message tests (DESIGN.md section 7 maps them to test ids):
  1  scene_bp_sweep / scene_bp_sweep_fixed, messages given, real accumulator
  2  ... first_sweep (msgs_in == nullptr), real accumulator
  3  ... uniform_acc with messages           4  ... first_sweep + uniform_acc (const_o, unbiased)
  5  scene_run(SWEEP, 0) on a float and on a fixed plan (uniform + biased, const_o, a0 = prior)
  6  scene_run(SWEEP, 1 | 2) on a float plan (STEADY: sums + prior)
  7  scene_run(SWEEP [| COMBINE], 1) on a fixed plan (messages, unbiased, not STEADY)
Buffers no route may read hold NaN (the other accumulator of a plan, the padding cells of a
bricked accumulator, the messages of a sweep without messages, a uniform accumulator beyond its
entry 0); what no route may write holds a sentinel and is compared bit for bit afterwards."""
import functools

import numpy as np
import pytest

import mrf_bwd_truth as T
import resident_truth as R
import scatter_truth as ST

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
f32 = np.float32
SENTINEL = f32(1234.5)          # beyond a row's count: never read, never written
PREFILL = f32(7.0)              # in a partial accumulator: a missed stripe of the clearing loop
ROWS = 256                      # rows of a launch, padded with rvc = 0 rows (a plan's row group)
PIXELS, RAYS = 300, 200         # a plan's pixel-order map and its rays per image (< ROWS)
CC = np.array([-3.1, 0.35, -0.2], f32)
CC_LONG = np.array([-55.0, 0.3, -0.2], f32)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    from raynet_amd import _lib
    _lib.build()
    return torch


@pytest.fixture(scope="module")
def contexts(torch, oracle_mod):
    """One context per (M, grid), made on first use: -> get(M, grid, bbox) -> (ctx, centers)."""
    from raynet_amd.hip_implementations.context import HipContext
    made = {}

    def get(M, grid=R.GRID, bbox=R.BBOX):
        if (M, grid) not in made:
            ctx = HipContext(M, 8, 2, 4, 8, 8, 3, bbox, grid)
            centers = oracle_mod.voxel_grid_centers(bbox, grid)
            ctx.set_voxel_grid(torch.from_numpy(centers).cuda())
            assert ctx.acc_size() == R.acc_size(grid)
            made[(M, grid)] = (ctx, centers)
        return made[(M, grid)]
    return get


# ------------------------------------------------------------------ host side
def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def rows_of(p, what, rows=ROWS, place=None, fill=0):
    """A launch's [n][...] array in a buffer of `rows` rows, launch row j at place[j]."""
    a = np.asarray(p[what] if isinstance(what, str) else what)
    place = np.arange(len(a)) if place is None else place
    out = np.full((rows,) + a.shape[1:], fill, a.dtype)
    out[place] = a
    return out


def live_rows(p, rows=ROWS, place=None):
    return rows_of(p, R.live(p), rows, place, False)


def messages_in(p, msgs, rows=ROWS, place=None):
    """The message buffer before a sweep: `msgs` on the entries a sweep reads (None: NaN, a sweep
    without messages reads none), the sentinel everywhere else."""
    inside = rows_of(p, np.arange(p["M"])[None, :] < R.counts_of(p)[:, None], rows, place, False)
    given = np.full(inside.shape, np.nan, f32) if msgs is None else rows_of(p, msgs, rows, place)
    return np.where(inside, given, SENTINEL).astype(f32)


@functools.lru_cache(maxsize=None)
def bp_truth(M, regime, form, grid=R.GRID, low=None):
    """(messages [n][M], sums [gx][gy][gz]) of one sweep in float64, per accumulator form."""
    p = R.bp_launch(M, regime, grid, low)
    zero = np.zeros_like(p["msgs"])
    acc, msgs = {"acc": (p["acc"], p["msgs"]), "first": (p["acc_first"], zero),
                 "uniform": (R.uniform(p["a0"], grid), p["msgs_uniform"]),
                 "uniform-first": (R.uniform(p["a0"], grid), zero),
                 "prior": (R.uniform(R.PRIOR, grid), zero), "eff": (p["acc_eff"], p["msgs"])}[form]
    return T.sweep_fwd(p["Sr"], p["rvi"], R.counts_of(p), acc, msgs)


def check_messages(what, p, got, before, truth, place=None):
    """The project's bound for this body on the live entries, every message finite; everything
    else -- beyond a row's count, rows of count <= 1, padding rows -- is what it was, bit for bit."""
    place = np.arange(len(p["rvc"])) if place is None else place
    live = R.live(p)
    g = got[place].astype(np.float64)
    assert np.isfinite(g[live]).all(), "%s: a message is not finite" % what
    bound = 1e-3 + 32 * EPS * (2 + np.exp(np.minimum(np.abs(truth), 30)))
    ratio = np.where(live, np.abs(np.where(live, g, 0) - truth) / bound, 0)
    r, i = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s: worst err / bound %.3g (row of %d voxels, entry %d, body %s)" % (
        what, ratio.max(), R.counts_of(p)[r], i, R.body_of(p["rvc"][r], p["M"])))
    assert ratio.max() <= 1, "%s: row of %d voxels, entry %d: got %r, truth %r, %d entries beyond the bound" % (
        what, R.counts_of(p)[r], i, g[r, i], truth[r, i], (ratio > 1).sum())
    keep = ~live_rows(p, len(got), place)
    assert np.array_equal(bits(got)[keep], bits(before)[keep]), \
        "%s: an entry beyond a row's count (or of a skipped row) was written" % what


def check_float_partial(what, p, part, msgs_got, place=None, padding=0.0):
    """A bricked float partial within the bound of its additions of exactly these messages:
    1.01 (n_v + 1) 2^-24 sum |m| per voxel; the padding cells hold `padding`."""
    place = np.arange(len(p["rvc"])) if place is None else place
    grid = p["grid"]
    truth, n_v, a_v = ST.partial_f64(msgs_got[place], p["rvi"], R.counts_of(p), grid)
    got = R.from_bricks(part, grid).astype(np.float64)
    err, bound = np.abs(got - truth), 1.01 * (n_v + 1) * EPS * a_v
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
    w = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s: sums worst err / bound %.3g at %s (n_v %d)" % (what, ratio.max(), w, n_v[w]))
    assert np.all(got[n_v == 0] == 0), "%s: a voxel no ray lists is not 0 (largest %g)" % (
        what, np.abs(got[n_v == 0]).max())
    assert np.all(err <= bound), "%s: voxel %s: got %r, truth %r (off by %g), bound %g" % (
        what, w, got[w], truth[w], got[w] - truth[w], bound[w])
    pad = part[R.padding_mask(grid)]
    assert np.all(pad == f32(padding)), "%s: padding cells hold %s, not %g" % (what, np.unique(pad)[:4], padding)


def check_fixed_partial(what, p, part, msgs_got, place=None, padding=0):
    place = np.arange(len(p["rvc"])) if place is None else place
    grid = p["grid"]
    truth = ST.partial_fixed(msgs_got[place], p["rvi"], R.counts_of(p), grid)
    got = R.from_bricks(part, grid)
    bad = np.argwhere(got != truth)
    print("%s: %d voxels hit, %d differ" % (what, np.count_nonzero(truth), len(bad)))
    assert len(bad) == 0, "%s: %d voxels differ; first %s: got %d, truth %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], truth[tuple(bad[0])])
    assert np.all(part[R.padding_mask(grid)] == padding), "%s: padding cells were written" % what
    return truth


# ------------------------------------------------------------------ device side
class Launch(object):
    """A launch's rows on the device, in a buffer of `rows` rows."""

    def __init__(self, torch, ctx, p, rows=ROWS, place=None):
        self.torch, self.ctx, self.p, self.rows = torch, ctx, p, rows
        self.place = np.arange(len(p["rvc"])) if place is None else place
        self.Sr = self.dev(rows_of(p, "Sr", rows, self.place))
        self.vox = self.dev(rows_of(p, "vox", rows, self.place))
        self.rvc = self.dev(rows_of(p, "rvc", rows, self.place))

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def messages(self, msgs):
        before = messages_in(self.p, msgs, self.rows, self.place)
        return before, self.dev(before)

    def bricked(self, acc, fill=np.nan):
        return self.dev(R.to_bricks(np.asarray(acc, f32), fill))

    def only_entry_0(self, value):
        a = np.full(self.ctx.acc_size(), np.nan, f32)
        a[0] = value
        return self.dev(a)

    def partial(self, fixed, cells, padding):
        a = np.full(self.ctx.acc_size(), cells, np.int64 if fixed else f32)
        a[R.padding_mask(self.p["grid"])] = padding
        return self.dev(a)

    def plan(self, msgs, acc0, acc1, fixed=None, n_images=1, depth_image=None, rays=None, ray_idxs=None):
        t = self.torch
        rpi = self.rows // n_images
        if ray_idxs is None:
            ray_idxs = np.arange(rpi if rays is None else rays, dtype=np.int32)
        self.depth = t.full((self.rows,), -1.0, device="cuda")
        cams = np.zeros((n_images, 12 * 2 + 16), f32)
        cams[:, 36:39] = centres_of(n_images, self.p["grid"])
        return self.ctx.scene_plan(n_images, rpi, self.dev(ray_idxs),
                                   t.zeros((n_images, 2), dtype=t.int64, device="cuda"), self.dev(cams),
                                   self.vox, self.rvc, self.Sr, msgs, acc0, acc1, self.depth, float(R.PRIOR),
                                   False, acc_fixed=fixed, depth_image=depth_image)


def centres_of(n, grid):
    """Camera centres outside the box, a different one per image (or group of rays)."""
    base = CC if grid == R.GRID else CC_LONG
    return (base[None, :] + np.arange(n)[:, None] * np.array([-0.7, 0.45, 0.3], f32)).astype(f32)


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------ a, b: messages and sums
def run_entry_routes(torch, ctx, p, truth_of, routes, what):
    L = Launch(torch, ctx, p)
    table = {1: ("acc", p["msgs"], lambda: L.bricked(p["acc"]), False, False),
             2: ("first", None, lambda: L.bricked(p["acc_first"]), True, False),
             3: ("uniform", p["msgs_uniform"], lambda: L.only_entry_0(p["a0"]), False, True),
             4: ("uniform-first", None, lambda: L.only_entry_0(p["a0"]), True, True)}
    for route in routes:
        form, msgs, acc_in, first, uni = table[route]
        truth = truth_of(form)[0]
        for fixed in (False, True):
            name = "%s route %d %s" % (what, route, "fixed" if fixed else "float")
            before, m = L.messages(msgs)
            # (no clearing on this route: the voxels' cells start at 0, the padding cells keep a mark)
            part = L.partial(fixed, 0, 5)
            run = ctx.scene_bp_sweep_fixed if fixed else ctx.scene_bp_sweep
            run(L.Sr, L.vox, L.rvc, acc_in(), m, part, first_sweep=first, uniform_acc=uni)
            torch.cuda.synchronize()
            got = host(m)
            check_messages(name, p, got, before, truth)
            if fixed:
                check_fixed_partial(name, p, host(part), got, padding=5)
            else:
                check_float_partial(name, p, host(part), got, padding=5.0)


@pytest.mark.parametrize("M,regime", R.BP_CASES)
def test_messages_through_the_sweep_entry_points(torch, contexts, M, regime):
    """Routes 1 - 4, float and fixed-point sums."""
    ctx, _ = contexts(M)
    p = R.bp_launch(M, regime)
    run_entry_routes(torch, ctx, p, lambda form: bp_truth(M, regime, form), (1, 2, 3, 4),
                     "M %d %s" % (M, regime))


@pytest.mark.parametrize("M,regime", R.BP_CASES)
def test_messages_through_a_float_plan(torch, contexts, M, regime):
    """Routes 5 (iteration 0: const_o with a0 = prior) and 6 (iterations 1 and 2: STEADY, the
    buffer holds sums).  The sweep clears the buffer it adds into inside k_bp: prefilled with 7."""
    from raynet_amd import _lib
    ctx, _ = contexts(M)
    p = R.bp_launch(M, regime)
    L = Launch(torch, ctx, p)
    G = ctx.acc_size()
    nan = np.full(G, np.nan, f32)
    for it in (0, 1, 2):
        name = "M %d %s route %d float plan, iteration %d" % (M, regime, 5 if it == 0 else 6, it)
        before, m = L.messages(None if it == 0 else p["msgs"])
        read = L.dev(nan) if it == 0 else L.bricked(p["sums"])
        read_before = host(read)
        write = L.partial(False, PREFILL, PREFILL)
        acc = [None, None]
        acc[(it + 1) & 1], acc[it & 1] = read, write
        pl = L.plan(m, acc[0], acc[1])
        ctx.scene_run(pl, _lib.RN_RUN_SWEEP, it)
        torch.cuda.synchronize()
        got = host(m)
        check_messages(name, p, got, before, bp_truth(M, regime, "prior" if it == 0 else "eff")[0])
        check_float_partial(name, p, host(write), got, padding=0.0)
        assert same_bits(host(read), read_before), "%s: the accumulator it reads was written" % name


@pytest.mark.parametrize("M,regime", R.BP_CASES)
def test_messages_through_a_fixed_plan(torch, contexts, M, regime):
    """Routes 5 (iteration 0) and 7 (iteration 1: messages, a full accumulator, not STEADY) with
    fixed-point sums; COMBINE turns them into prior + sum and clears them."""
    from raynet_amd import _lib
    ctx, _ = contexts(M)
    p = R.bp_launch(M, regime)
    L = Launch(torch, ctx, p)
    G = ctx.acc_size()
    nan = np.full(G, np.nan, f32)
    pad = R.padding_mask(p["grid"])
    for it, phases in ((0, _lib.RN_RUN_SWEEP), (1, _lib.RN_RUN_SWEEP),
                       (1, _lib.RN_RUN_SWEEP | _lib.RN_RUN_COMBINE)):
        combine = bool(phases & _lib.RN_RUN_COMBINE)
        name = "M %d %s route %d fixed plan, iteration %d%s" % (M, regime, 5 if it == 0 else 7, it,
                                                                 " + combine" if combine else "")
        before, m = L.messages(None if it == 0 else p["msgs"])
        read = L.dev(nan) if it == 0 else L.bricked(p["acc"])
        read_before = host(read)
        other = L.partial(False, PREFILL, PREFILL)
        acc = [None, None]
        acc[(it + 1) & 1], acc[it & 1] = read, other
        sums = torch.zeros((G,), dtype=torch.int64, device="cuda")
        pl = L.plan(m, acc[0], acc[1], fixed=sums)
        ctx.scene_run(pl, phases, it)
        torch.cuda.synchronize()
        got = host(m)
        check_messages(name, p, got, before, bp_truth(M, regime, "prior" if it == 0 else "acc")[0])
        assert same_bits(host(read), read_before), "%s: the accumulator it reads was written" % name
        if not combine:
            check_fixed_partial(name, p, host(sums), got)
            assert np.all(host(other) == PREFILL), "%s: a fixed-point sweep wrote a float accumulator" % name
            plain = got
        else:
            assert same_bits(got, plain), "%s: other messages than without COMBINE" % name
            assert not host(sums).any(), "%s: COMBINE left sums behind" % name
            fixed = ST.partial_fixed(got, p["rvi"], R.counts_of(p), p["grid"])
            want = f32(R.PRIOR) + (fixed.astype(np.float64) * 2.0 ** -32).astype(f32)
            out = host(other)
            assert same_bits(R.from_bricks(out, p["grid"]), want.astype(f32)), "%s: prior + sum" % name
            assert np.all(out[pad] == f32(R.PRIOR))


# ------------------------------------------------------------------ c: depth
@functools.lru_cache(maxsize=None)
def depth_d(M, regime, form, grid=R.GRID, low=None):
    """The float64 distribution, its first arg-max and top-2 gap (no geometry in these)."""
    p = R.depth_launch(M, regime, grid, low)
    return R.depth_truth(p, p[form], p["msgs"], np.zeros(tuple(grid) + (3,), f32), np.zeros(3, f32))


def check_distribution(what, p, S, truth):
    counts, live = R.counts_of(p), R.live(p)
    n = len(counts)
    g = S[:n].astype(np.float64)
    err = np.where(live, np.abs(np.where(live, g, 0) - truth["d"]), 0)
    total = np.where(live, g, 0).sum(1)
    print("%s: distribution worst err %.3g (bound %g), worst |sum - 1| %.3g" % (
        what, err.max(), R.D_TOL, np.abs(total - 1)[counts > 1].max()))
    assert np.isfinite(g[live]).all()
    assert err.max() <= R.D_TOL, "%s: row of %d voxels" % (what, counts[np.unravel_index(err.argmax(), err.shape)[0]])
    assert np.abs(total - 1)[counts > 1].max() <= 1e-5
    inside = np.arange(p["M"])[None, :] < counts[:, None]
    assert np.all(S[:n][inside & ~live] == 0), "%s: a skipped ray's first `count` entries are not 0" % what
    assert np.all(S[:n][~inside] == SENTINEL) and np.all(S[n:] == SENTINEL), \
        "%s: an entry beyond a row's count was written" % what


def check_depth(what, p, depth, truth, centers, cc_rows, only=None):
    """depth [n]: on rows with one sure arg-max the distance of THAT voxel within 8 * 2^-24 t
    (three rounded differences, three squares, two additions, a square root, each <= 2^-24
    relative on positive terms); on the others, of some voxel whose truth lies within 1e-4 of the
    maximum.  An empty list reports voxel (0, 0, 0), a list of one its voxel.  only [n] bool: the
    rows this launch covers."""
    counts = R.counts_of(p)
    t64 = R.t64_of(p["rvi"], centers, cc_rows)
    t0 = R.t64_of(np.zeros((len(counts), 1, 3), np.int64), centers, cc_rows)[:, 0]
    worst = 0.0
    for r, c in enumerate(counts):
        if only is not None and not only[r]:
            continue
        got = float(depth[r])
        if c <= 1:
            want = [t0[r] if c == 0 else t64[r, 0]]
        elif truth["sure"][r]:
            want = [t64[r, truth["arg"][r]]]
        else:
            d = truth["d"][r, :c]
            want = t64[r, :c][d >= d.max() - 1e-4]
        ratio = min(abs(got - t) / (8 * EPS * t) for t in want)
        worst = max(worst, ratio)
        assert ratio <= 1, "%s: row %d of %d voxels (%s, body %s): depth %r, truth %r (arg-max %d, gap %g)" % (
            what, r, c, p["kinds"][r], R.body_of(c, p["M"]), got, want[0], truth["arg"][r], truth["gap"][r])
    print("%s: depth worst err / bound %.3g" % (what, worst))


def run_depth_entry_routes(torch, ctx, centers, p, truth, what, all_routes=True):
    L = Launch(torch, ctx, p)
    n = len(p["rvc"])
    acc = L.bricked(p["acc"])
    before, m = L.messages(p["msgs"])
    cc = centres_of(1, p["grid"])[0]
    cc_rows = np.repeat(cc[None], n, 0)
    new = lambda: torch.full((ROWS, p["M"]), float(SENTINEL), device="cuda")
    depth_of = lambda: torch.full((ROWS,), -1.0, device="cuda")
    # the distribution and the depth
    S, depth = new(), depth_of()
    ctx.scene_depth(L.Sr, L.vox, L.rvc, acc, m, L.dev(cc), S, depth)
    torch.cuda.synchronize()
    S, depth = host(S), host(depth)
    check_distribution(what + " S_new + depth", p, S, truth)
    check_depth(what + " S_new + depth", p, depth, truth, centers, cc_rows)
    t_origin = R.t64_of(np.zeros((1, 1, 3), np.int64), centers, cc)[0, 0]
    assert np.all(np.abs(depth[n:] - t_origin) <= 8 * EPS * t_origin)        # (padding rows: empty lists)
    assert same_bits(host(m), before)
    if not all_routes:
        return
    # the distribution alone
    S2 = new()
    ctx.scene_depth(L.Sr, L.vox, L.rvc, acc, m, None, S2, None)
    assert same_bits(host(S2), S), "%s: S_new alone is another distribution" % what
    # the depth alone: the same instantiation, only the store skipped
    d3 = depth_of()
    ctx.scene_depth(L.Sr, L.vox, L.rvc, acc, m, L.dev(cc), None, d3)
    assert same_bits(host(d3), depth), "%s: the depth alone differs from the depth next to S_new" % what
    # groups of 64 rows, each with a camera centre of its own
    groups = ROWS // 64
    table = np.zeros((groups, 4), f32)
    table[:, :3] = centres_of(groups, p["grid"])
    S4, d4 = new(), depth_of()
    ctx.scene_depth(L.Sr, L.vox, L.rvc, acc, m, L.dev(table), S4, d4, rays_per_center=64)
    torch.cuda.synchronize()
    assert same_bits(host(S4), S)
    check_depth(what + " rays_per_center 64", p, host(d4), truth, centers, table[np.arange(n) // 64, :3])
    # the statistics sweep: the same depth and distribution, and the confidence IS the maximum
    S5, d5 = new(), depth_of()
    stats = torch.full((3, ROWS + 5), -7.0, device="cuda")
    ctx.scene_depth_stats(L.Sr, L.vox, L.rvc, acc, m, L.dev(cc), S5, d5, stats)
    torch.cuda.synchronize()
    S5, st = host(S5), host(stats)
    check_distribution(what + " stats", p, S5, truth)
    check_depth(what + " stats", p, host(d5), truth, centers, cc_rows)
    assert same_bits(S5, S) and same_bits(host(d5), depth), "%s: k_depth_stats differs from k_depth" % what
    live = R.counts_of(p) > 1
    conf = np.where(R.live(p), S5[:n], -np.inf).max(1)
    assert same_bits(st[0, :n][live], conf[live].astype(f32)), "%s: confidence is not the row's maximum" % what
    assert np.all(st[:, ROWS:] == -7.0) and np.isfinite(st[:, :ROWS]).all()
    assert same_bits(host(m), before)


@pytest.mark.parametrize("M,regime", R.DEPTH_CASES)
def test_depth_through_the_entry_points(torch, contexts, M, regime):
    """scene_depth with S_new and / or depth_map, with rays_per_center, and scene_depth_stats."""
    ctx, centers = contexts(M)
    run_depth_entry_routes(torch, ctx, centers, R.depth_launch(M, regime), depth_d(M, regime, "acc"),
                           "M %d %s" % (M, regime))


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "fixed"])
@pytest.mark.parametrize("M,regime", R.DEPTH_CASES)
def test_depth_through_a_plan(torch, contexts, M, regime, fixed):
    """scene_run with DEPTH (all images, one image) and DEPTH_RANGE on a float plan (STEADY: sums
    + prior, no distribution) and on a fixed plan (a full accumulator), in row order and in pixel
    order.  Two images of 256 rows, 200 rays each; the launch's rows alternate between them."""
    from raynet_amd import _lib
    ctx, centers = contexts(M)
    p = R.depth_launch(M, regime)
    truth = depth_d(M, regime, "acc" if fixed else "acc_eff")
    n = len(p["rvc"])
    rows, rpi = 2 * ROWS, ROWS
    place = (np.arange(n) % 2) * rpi + np.arange(n) // 2
    assert place.max() % rpi < RAYS
    L = Launch(torch, ctx, p, rows, place)
    cc2 = centres_of(2, p["grid"])
    cc_rows = cc2[np.arange(n) % 2]
    before, m = L.messages(p["msgs"])
    read = L.bricked(p["acc"] if fixed else p["sums"])
    nan = L.dev(np.full(ctx.acc_size(), np.nan, f32))
    sums = torch.zeros((ctx.acc_size(),), dtype=torch.int64, device="cuda") if fixed else None
    ray_idxs = np.random.default_rng(M).permutation(PIXELS)[:RAYS].astype(np.int32)
    t_origin = R.t64_of(np.zeros((2, 1, 3), np.int64), centers, cc2)[:, 0]
    what = "M %d %s %s plan" % (M, regime, "fixed" if fixed else "float")
    routes = (("all images", _lib.RN_RUN_DEPTH, -1, (0, 1), rpi),
              ("range", _lib.RN_RUN_DEPTH_RANGE, 1 | (1 << 16), (1,), rpi),
              ("one image", _lib.RN_RUN_DEPTH, 0, (0,), RAYS))
    for name, phases, image, images, written in routes:
        # row order: iteration 1 reads acc[0]; acc[1] is never read
        pl = L.plan(m, read, nan, fixed=sums, n_images=2, rays=RAYS, ray_idxs=ray_idxs)
        ctx.scene_run(pl, phases, 1, image)
        torch.cuda.synchronize()
        depth = host(L.depth)
        wrote = np.zeros(rows, bool)
        for g in images:
            wrote[g * rpi:g * rpi + written] = True
        assert np.all(depth[~wrote] == -1.0), "%s %s: rows of another image (or padding rows) were written" % (what, name)
        check_depth("%s %s" % (what, name), p, depth[place], truth, centers, cc_rows, only=wrote[place])
        empty = wrote & ~rows_of(p, R.counts_of(p) > 0, rows, place, False)
        for g in images:
            e = depth[g * rpi:(g + 1) * rpi][empty[g * rpi:(g + 1) * rpi]]
            assert np.all(np.abs(e - t_origin[g]) <= 8 * EPS * t_origin[g])
        # pixel order: the same bits at depth_image[g][ray_idxs[row]], nothing else written
        image_map = torch.full((2, PIXELS), -2.0, device="cuda")
        pl = L.plan(m, read, nan, fixed=sums, n_images=2, depth_image=image_map, rays=RAYS, ray_idxs=ray_idxs)
        ctx.scene_run(pl, phases, 1, image)
        torch.cuda.synchronize()
        got_map = host(image_map)
        want_map = np.full((2, PIXELS), -2.0, f32)
        for g in images:
            want_map[g, ray_idxs] = depth[g * rpi:g * rpi + RAYS]
        assert same_bits(got_map, want_map), "%s %s: the pixel-order map is not the row-order map permuted" % (what, name)
        assert np.all(host(L.depth) == -1.0), "%s %s: row-order depths written next to a pixel-order map" % (what, name)
    assert same_bits(host(m), before) and np.isnan(host(nan)).all()
    if fixed:
        assert not host(sums).any()


# ------------------------------------------------------------------ d: the brick layout
def test_brick_layout_on_the_long_grid(torch, contexts):
    """acc_from_grid / acc_to_grid on (1021, 5, 6) against resident_truth's layout, bit for bit."""
    ctx, _ = contexts(R.M_LONG, R.GRID_LONG, R.BBOX_LONG)
    rng = np.random.default_rng(5)
    a = rng.standard_normal(R.GRID_LONG).astype(f32)
    v = host(ctx.acc_from_grid(torch.from_numpy(a).cuda()))
    assert same_bits(v, R.to_bricks(a, 0.0))
    w = rng.standard_normal(R.acc_size(R.GRID_LONG)).astype(f32)
    w[R.padding_mask(R.GRID_LONG)] = np.nan
    back = host(ctx.acc_to_grid(torch.from_numpy(w).cuda()))
    assert same_bits(back, R.from_bricks(w, R.GRID_LONG).astype(f32))


@pytest.mark.parametrize("low", R.LONG_CASES, ids=["x-below-8", "x-from-1000"])
def test_sweeps_at_both_ends_of_the_long_axis(torch, contexts, low):
    """Route 1 and the first depth route on lists from x < 8 and from x >= 1000 (brick
    x-coordinates 250 .. 255: the 8-bit fields of lin_of)."""
    ctx, centers = contexts(R.M_LONG, R.GRID_LONG, R.BBOX_LONG)
    M, grid = R.M_LONG, R.GRID_LONG
    p = R.bp_launch(M, "mixed", grid, low)
    run_entry_routes(torch, ctx, p, lambda form: bp_truth(M, "mixed", form, grid, low), (1,),
                     "long grid, low %s" % low)
    run_depth_entry_routes(torch, ctx, centers, R.depth_launch(M, "empty", grid, low),
                           depth_d(M, "empty", "acc", grid, low), "long grid, low %s" % low, all_routes=False)
