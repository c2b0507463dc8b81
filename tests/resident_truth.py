"""Fixtures and float64 truths for the RESIDENT BP and depth sweeps (packed voxel words, 4x4x4
bricked accumulators, columns already clipped): k_bp<NCH, true, false, STEADY>, k_depth<...> and
k_depth_stats of csrc/raynet_mrf.inl.  No GPU in here; tests/test_resident_truth.py holds every
function to closed forms and asserts the conditions on the fixtures,
tests/test_resident_sweeps_gpu.py runs the kernels on them.

The mathematics is that of tests/mrf_bwd_truth.py (sweep_fwd, depth_fwd, make_launch,
check_launch and its regimes), reused and not restated.  What is added: the counts of a launch
that reach every per-ray body and both edges of every chunk, the packed / bricked layouts, the
biased (sums + prior) and uniform accumulator forms, and depth columns with a known arg-max.

Body of a ray (RN_DISPATCH_CHUNKS): a launch is compiled for NCH = the smallest of 2, 4, 6, 8, 12,
16 that holds ceil(M / 64) chunks; a ray of nch = ceil(count / 64) chunks runs the body NB = the
smallest of 1, 2, 3, 4, 6, 8, 12 that is >= nch and <= NCH, else NCH.  So chunk counts 5, 7, 9-11
and 13-15 run a body with dead chunks."""
import functools

import numpy as np

import mrf_bwd_truth as T

f32 = np.float32
MS = (128, 256, 384, 512, 768, 1024)
GRID = (13, 10, 9)              # no axis a multiple of 4: 4 x 3 x 3 bricks, 1170 voxels
BBOX = np.array([-1.3, -1.0, -0.9, 1.3, 1.0, 0.9], f32)
GRID_LONG = (1021, 5, 6)        # brick x-coordinates up to 255: the 8-bit fields of lin_of
BBOX_LONG = np.array([-51.05, -0.5, -0.6, 51.05, 0.5, 0.6], f32)
M_LONG = 128
PRIOR = f32(np.log(0.05 / 0.95))        # log-odds of gamma = 0.05: about -2.944
LAUNCH_CHUNKS = (2, 4, 6, 8, 12, 16)
BODIES = (1, 2, 3, 4, 6, 8, 12)
ALL_BODIES = (1, 2, 3, 4, 6, 8, 12, 16)
KINDS = ("broad", "sharp", "last", "first")
D_TOL = 5e-5                    # the distribution bound of the GPU tests
SURE_GAP = 2 * D_TOL            # a row whose float64 top-2 gap is above this has ONE arg-max


# the cases of tests/test_resident_sweeps_gpu.py: (M, regime)
BP_CASES = tuple((M, regime) for M in MS for regime in T.REGIMES)
DEPTH_CASES = tuple((M, "empty") for M in MS) + ((384, "prior"), (384, "saturated"))
LONG_CASES = (True, False)      # GRID_LONG at M_LONG: lists from x < 8, from x >= 1000


# ------------------------------------------------------------------ launches and bodies
def rows_for(M):
    """The counts of one launch: skipped rays, both edges of every chunk, the full row.  (The
    fixtures add one more row of M entries whose rvc is M + 7: the kernels clamp to M.)"""
    counts = [0, 1, 2, 3]
    for k in range(1, M // 64 + 1):
        counts += [64 * k - 1, 64 * k]
        if 64 * k + 1 <= M:
            counts.append(64 * k + 1)
    counts.append(M)
    return counts


def launch_class(M):
    nch = -(-int(M) // 64)
    return next(c for c in LAUNCH_CHUNKS if c >= nch)


def body_of(count, M):
    """NB of the per-ray body a ray of `count` voxels runs in a launch of row length M (None for
    a ray the kernels skip)."""
    count = min(int(count), int(M))
    if count <= 1:
        return None
    nch, NCH = -(-count // 64), launch_class(M)
    for b in BODIES:
        if NCH >= b and nch <= b:
            return b
    return NCH


def last_live_chunk(count, M):
    return (min(int(count), int(M)) - 1) // 64


# ------------------------------------------------------------------ packing and bricks
def pack(rvi):
    rvi = np.asarray(rvi)
    return ((rvi[..., 0] << 20) | (rvi[..., 1] << 10) | rvi[..., 2]).astype(np.int32)


def bricks_of(grid):
    return tuple((int(g) + 3) // 4 for g in grid)


def acc_size(grid):
    return int(np.prod(bricks_of(grid))) * 64


def brick_index(grid, x, y, z):
    """Offset of voxel (x, y, z) in the layout [ceil(gx/4)][ceil(gy/4)][ceil(gz/4)][4][4][4]."""
    x, y, z = (np.asarray(a).astype(np.int64) for a in (x, y, z))
    _, nby, nbz = bricks_of(grid)
    brick = ((x // 4) * nby + y // 4) * nbz + z // 4
    return brick * 64 + (x % 4) * 16 + (y % 4) * 4 + z % 4


def _all_offsets(grid):
    X, Y, Z = np.meshgrid(*[np.arange(int(g)) for g in grid], indexing="ij")
    return brick_index(grid, X, Y, Z)


def to_bricks(a, fill=0):
    """[gx][gy][gz] -> the bricked vector, padding cells holding `fill`."""
    a = np.asarray(a)
    out = np.full(acc_size(a.shape), fill, a.dtype)
    out[_all_offsets(a.shape)] = a
    return out


def from_bricks(v, grid):
    return np.asarray(v).ravel()[_all_offsets(grid)]


def padding_mask(grid):
    """True at the cells of the bricked vector that are no voxel's."""
    m = np.ones(acc_size(grid), bool)
    m[_all_offsets(grid).ravel()] = False
    return m


# ------------------------------------------------------------------ accumulator forms
def biased(acc, prior=PRIOR):
    """A plan's float accumulator holds the messages' sums and the prior is added at the gather:
    -> (sums, acc_eff) with sums = f32(acc - f32(prior)) and acc_eff = f32(f32(prior) + sums),
    the value the kernel forms and the one the truth is evaluated on."""
    acc = np.asarray(acc, f32)
    sums = (acc - f32(prior)).astype(f32)
    return sums, (f32(prior) + sums).astype(f32)


def uniform(value, grid):
    """The truth's accumulator when every voxel holds one value."""
    return np.full(tuple(grid), f32(value), f32)


def out_of_band(acc):
    """The accumulator of a sweep WITHOUT messages (mu = acc itself): entries whose magnitude lies
    in the band are moved below it, to 8.2 .. 8.6, keeping their sign and order."""
    acc = np.asarray(acc, f32)
    lo, hi = T.BAND
    moved = np.sign(acc) * (8.2 + 0.4 * (np.abs(acc) - lo) / (hi - lo))
    return np.where(T._in_band(acc), moved, acc).astype(f32)


def counts_of(p):
    """The counts the kernels use: rvc clamped to the row length."""
    return np.minimum(p["rvc"], p["M"]).astype(np.int32)


def live(p):
    c = counts_of(p)
    return np.arange(p["M"])[None, :] < np.where(c > 1, c, 0)[:, None]


def _voxel_values(p, acc):
    lin = np.ravel_multi_index(tuple(np.moveaxis(p["rvi"].astype(np.int64), -1, 0)), p["grid"])
    return np.asarray(acc).ravel()[lin]


def band_free(p, acc, msgs):
    """No |mu| of a listed entry in mrf_bwd_truth.BAND, in fp32 or in float64."""
    a = _voxel_values(p, acc)
    m = np.asarray(msgs)
    inside = np.arange(p["M"])[None, :] < counts_of(p)[:, None]
    for mu in (a - m, a.astype(np.float64) - m):
        if T._in_band(mu[inside]).any():
            return False
    return True


def messages_for_uniform(p, value):
    """Messages that give the launch's own mu against an accumulator of `value` everywhere:
    f32(value - (acc[voxel] - msgs)); zero beyond the counts."""
    mu = _voxel_values(p, p["acc"]).astype(np.float64) - p["msgs"]
    inside = np.arange(p["M"])[None, :] < counts_of(p)[:, None]
    return np.where(inside, float(value) - mu, 0.0).astype(f32)


def _finish(p, M, seed):
    """The row whose rvc is beyond M, and the derived forms every route needs."""
    p["M"] = int(M)
    p["seed"] = seed
    counts = p["rvc"].tolist()
    T.check_launch(p, counts, M)
    p["rvc"] = p["rvc"].copy()
    p["rvc"][-1] = M + 7                      # the list stays M long: the kernels clamp
    p["vox"] = pack(p["rvi"])
    p["sums"], p["acc_eff"] = biased(p["acc"])
    p["a0"] = f32(p["acc"][0, 0, 0])          # bricked entry 0: what a uniform sweep reads
    p["msgs_uniform"] = messages_for_uniform(p, p["a0"])
    p["acc_first"] = out_of_band(p["acc"])
    q = dict(p, acc=p["acc_eff"], rvc=np.asarray(counts, np.int32))
    ok = band_free(p, p["acc_eff"], p["msgs"]) and band_free(p, uniform(p["a0"], p["grid"]), p["msgs_uniform"]) \
        and not T._in_band(np.array([p["a0"], PRIOR], np.float64)).any()
    if ok:
        T.check_launch(q, counts, M)          # the biased form meets every condition too
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ok


@functools.lru_cache(maxsize=None)
def bp_launch(M, regime, grid=GRID, low=None):
    """The launch of the message tests at this M and regime (shared: do not modify).  A seed whose
    biased or uniform form puts an entry into the band is passed over, here on the CPU.
    low: draw every list from the voxels with x < 8 (True) or x >= 1000 (False) of GRID_LONG."""
    counts = rows_for(M) + [M]
    for attempt in range(20):
        seed = 7000 + 10 * M + 100000 * attempt + T.REGIMES.index(regime) + (0 if low is None else 5 + low)
        p = T.make_launch(counts, M, regime, seed, grid)
        if low is not None:
            _move_lists(p, low, seed)
        if _finish(p, M, seed):
            return p
    raise AssertionError("no seed keeps (M %d, %s) out of the band" % (M, regime))


def _move_lists(p, low, seed):
    """Redraw the lists of a GRID_LONG launch from one end of the x axis (the accumulator is
    random everywhere, the messages are shifted so that every mu stays what it was)."""
    gx, gy, gz = p["grid"]
    xs = np.arange(0, 8) if low else np.arange(1000, gx)
    rng = np.random.default_rng(seed + 1)
    pool = np.stack(np.meshgrid(xs, np.arange(gy), np.arange(gz), indexing="ij"), -1).reshape(-1, 3)
    mu = _voxel_values(p, p["acc"]).astype(np.float64) - p["msgs"]
    for r, c in enumerate(p["rvc"]):
        assert c <= len(pool)
        p["rvi"][r, :c] = pool[rng.choice(len(pool), c, replace=False)]
    a = _voxel_values(p, p["acc"])
    inside = np.arange(p["rvi"].shape[1])[None, :] < p["rvc"][:, None]
    p["msgs"][...] = np.where(inside, a.astype(np.float64) - mu, 0.0).astype(f32)


# ------------------------------------------------------------------ depth columns
def depth_columns(counts, kinds, M, seed):
    """Columns of the three kinds of tests/test_depth_statistics_gpu.py::_kernel_case (and `first`),
    clipped and renormalised as resident columns are.  `last` puts the peak into the row's last 20
    entries, `first` into its first 20."""
    rng = np.random.default_rng(seed)
    Sr = np.zeros((len(counts), M), f32)
    for r, (c, kind) in enumerate(zip(counts, kinds)):
        if c == 0:
            continue
        s = rng.random(c) + 0.05
        if kind == "sharp":
            s[int(rng.integers(0, c))] += 200.0 * c
        elif kind == "last":
            s[c - 1 - int(rng.integers(0, min(c, 20)))] += 200.0 * c
        elif kind == "first":       # (the mirror image of `last`: an arg-max in chunk 0 of a long row)
            s[int(rng.integers(0, min(c, 20)))] += 200.0 * c
        else:
            assert kind == "broad"
        Sr[r, :c] = T.clip_and_renorm_f32(s / s.sum())
    return Sr


def depth_rows(M):
    """(counts, kinds) of a depth launch: every count of rows_for(M) with a sharp and a `last`
    column, every sixth also with a broad one, and the full chunks also with a `first` one."""
    counts, kinds = [], []
    for j, c in enumerate(rows_for(M) + [M]):
        for kind in ("sharp", "last") + (("broad",) if j % 6 == 2 else ()) + \
                (("first",) if c and c % 64 == 0 else ()):
            counts.append(c)
            kinds.append(kind)
    return counts, kinds


@functools.lru_cache(maxsize=None)
def depth_launch(M, regime, grid=GRID, low=None):
    """The launch of the depth tests (shared: do not modify)."""
    counts, kinds = depth_rows(M)
    for attempt in range(20):
        seed = 9000 + 10 * M + 100000 * attempt + T.REGIMES.index(regime) + (0 if low is None else 5 + low)
        p = T.make_launch(counts, M, regime, seed, grid)
        if low is not None:
            _move_lists(p, low, seed)
        p["Sr"] = depth_columns(counts, kinds, M, seed + 2)
        p["kinds"] = tuple(kinds)
        if _finish(p, M, seed):
            return p
    raise AssertionError("no seed keeps (M %d, %s) out of the band" % (M, regime))


def t64_of(rvi, centers, cc):
    """float64 distance of every listed voxel's centre from the camera centre, from the fp32
    values the kernel reads: centers [gx][gy][gz][3] f32 (their per-axis values are the context's
    `axes`), cc [3] f32 or one per row [n][3]."""
    rvi = np.asarray(rvi)
    pts = np.asarray(centers, f32)[rvi[..., 0], rvi[..., 1], rvi[..., 2]].astype(np.float64)
    cc = np.asarray(cc, f32).astype(np.float64)
    if cc.ndim == 2:
        cc = cc[:, None, :]
    return np.sqrt(((pts - cc) ** 2).sum(-1))


def depth_truth(p, acc, msgs, centers, cc):
    """Per ray of the launch: d [n][M] the float64 distribution (T.depth_fwd), arg [n] the index
    of its first maximum, gap [n] the float64 distance between its two largest entries, t64
    [n][M].  Rays the kernels skip: d all zero, arg 0, gap 0 (the kernel reports voxel (0, 0, 0)
    for an empty list, the first voxel for a list of one)."""
    counts = counts_of(p)
    d = T.depth_fwd(p["Sr"], p["rvi"], counts, acc, msgs)
    n = len(counts)
    arg, gap = np.zeros(n, np.int64), np.zeros(n)
    for r in range(n):
        c = int(counts[r])
        if c > 1:
            arg[r] = int(np.argmax(d[r, :c]))
            top = np.sort(d[r, :c])[-2:]
            gap[r] = top[1] - top[0]
    return dict(d=d, arg=arg, gap=gap, t64=t64_of(p["rvi"], centers, cc), sure=gap > SURE_GAP)
