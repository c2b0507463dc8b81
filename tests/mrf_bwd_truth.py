"""Per-launch truths, an fp32 restatement and crafted inputs for the MRF training kernels
(k_ray_bwd<0>, k_ray_bwd<1>, and the training forward) of csrc/raynet_train.inl.  No GPU.

* sweep_fwd / sweep_bwd / depth_fwd / depth_bwd: ONE launch in float64, built from the pieces
  of oracle/mrf_backward.py (_ray_messages, _ray_messages_bwd, _chain_from_wbar) -- the
  mathematics is stated there and nowhere else.  They take the fp32 arrays the kernel gets.
  The accumulator is a [gx][gy][gz] array and a voxel's entry is (x * gy + y) * gz + z, what
  lin_of<false> computes for the training entry points.
* ray_bwd_fp32 / launch_fp32: k_ray_bwd's formulas line by line in NumPy float32, one rounding
  per operation, running sums and products taken sequentially.  NOT a second truth: it
  measures how much of the float64 value ANY fp32 evaluation of these formulas keeps, and the
  constants E_* below (its worst error per mode, output and regime, measured by
  tests/test_mrf_bwd_truth.py) are what the GPU tolerances are derived from.
* make_launch: crafted problems that need no traversal -- a row is a random set of distinct
  voxels of a 16^3 grid, so rows share voxels and g_acc receives sums from several rays.
"""
import functools

import numpy as np

from oracle import mrf_backward as mb

GRID = (16, 16, 16)
# mu = acc - msgs.  prior: around -3, occupancies near the prior; mixed: N(0, 2); saturated: mixed
# with a tenth of the entries at |mu| in [12, 20] (the occupancy clamp active, its derivative 0);
# empty: around -6.5, occupancies of ~1.5e-3, so that the transmittance is still 0.2 behind 1024
# voxels and EVERY chunk's carry of a long row matters (at the prior it has decayed to 1e-3
# behind 128 voxels, in the mixed regimes behind a few dozen)
REGIMES = ("prior", "mixed", "saturated", "empty")
# fp32 and float64 can disagree about whether the occupancy clamp (|mu| = ln 9999 = 9.21) is
# active only next to the switch; no crafted |mu| lies in this band
BAND = (8.7, 9.7)
FP32_LENGTHS = (2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 1023, 1024)
FP32_DRAWS = 6
# the launches of tests/test_mrf_backward_kernels_gpu.py: every count at which k_ray_bwd's chunk
# loops change (one, two, three chunks and their edges), skipped rays, each at least twice; at
# the library's largest M the shortest row and the two longest
GPU_COUNTS = {192: [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192] * 2 +
                   [64, 65, 128, 129, 192, 100, 17, 130],
              1024: [2, 1023, 1024] * 2}

# Worst error of the sequential fp32 restatement against the float64 truth, over FP32_LENGTHS
# x FP32_DRAWS rays per regime and the launches of gpu_launch, so that the factor between the
# restatement and the kernel is taken on the kernel's own inputs
# (test_fp32_restatement_error measures exactly these; the values
# are the measured ones rounded up to two digits; in brackets the measured value and the row
# length that produced it).  g_s and g_msgs: max|got - ref| over a ray / max|ref| over that
# ray.  g_acc: the same over a launch (its sums cross rays).  E_DEPTH_GS_SATURATED: over the
# launch too, see LAUNCH_WIDE.
E_SWEEP_GS_PRIOR = 2.8e-7         # [2.789e-07, row length 2]
E_SWEEP_GS_MIXED = 1.2e-6         # [1.130e-06, row length 63]
E_SWEEP_GS_SATURATED = 6.5e-6     # [6.468e-06, row length 128]
E_SWEEP_GS_EMPTY = 3.9e-7         # [3.814e-07, row length 2]
E_SWEEP_GMSGS_PRIOR = 8.3e-7      # [8.218e-07, the GPU launch at M = 1024]
E_SWEEP_GMSGS_MIXED = 4.3e-6      # [4.228e-06, the GPU launch at M = 1024]
E_SWEEP_GMSGS_SATURATED = 3.8e-6  # [3.737e-06, row length 3]
E_SWEEP_GMSGS_EMPTY = 5.1e-6      # [5.085e-06, row length 192]
E_SWEEP_GACC_PRIOR = 6.0e-7       # [5.997e-07, row length 1024]
E_SWEEP_GACC_MIXED = 8.1e-7       # [8.074e-07, the GPU launch at M = 1024]
E_SWEEP_GACC_SATURATED = 6.7e-7   # [6.607e-07, row length 127]
E_SWEEP_GACC_EMPTY = 1.4e-6       # [1.318e-06, row length 192]
E_DEPTH_GS_PRIOR = 2.0e-6         # [1.967e-06, row length 2]
E_DEPTH_GS_MIXED = 5.6e-5         # [5.531e-05, row length 128]
E_DEPTH_GS_SATURATED = 2.7e-6     # [2.633e-06, row length 1023]
E_DEPTH_GS_EMPTY = 2.0e-6         # [1.938e-06, the GPU launch at M = 192]
E_DEPTH_GMSGS_PRIOR = 9.6e-6      # [9.564e-06, row length 2]
E_DEPTH_GMSGS_MIXED = 6.1e-6      # [6.086e-06, row length 65]
E_DEPTH_GMSGS_SATURATED = 5.4e-6  # [5.363e-06, the GPU launch at M = 192]
E_DEPTH_GMSGS_EMPTY = 1.4e-5      # [1.330e-05, the GPU launch at M = 192]
E_DEPTH_GACC_PRIOR = 9.5e-7       # [9.437e-07, row length 1023]
E_DEPTH_GACC_MIXED = 6.5e-7       # [6.448e-07, row length 192]
E_DEPTH_GACC_SATURATED = 6.5e-7   # [6.413e-07, row length 63]
E_DEPTH_GACC_EMPTY = 1.4e-6       # [1.320e-06, row length 1023]

MODES = ("sweep", "depth")
OUTPUTS = ("gs", "gmsgs", "gacc")


def E(mode, output, regime):
    return globals()["E_%s_%s_%s" % (mode.upper(), output.upper(), regime.upper())]


# The one combination held against the largest |ref| of the LAUNCH instead of the ray's own:
# when a single voxel holds nearly all of a ray's weight (a saturated occupancy in front),
# d_i is ~1 there and g_i - sum_j g_j d_j cancels; that ray's whole dL/ds is then tiny and
# keeps few digits (up to 5e-3 of its own maximum in fp32), while against the launch's largest
# gradient the same data stays below 1e-6.
LAUNCH_WIDE = {("depth", "gs", "saturated")}
GPU_FACTOR = 16          # tree scans, chunk carries and the device's expf against a sequential sum


# ------------------------------------------------------------------ float64 truths
def _rays(rvi, rvc, grid):
    for r in range(len(rvc)):
        c = int(rvc[r])
        if c > 1:
            yield r, c, np.ravel_multi_index(tuple(rvi[r, :c].T.astype(np.int64)), grid)


def _f64(*arrays):
    """The fp32 arrays widened to float64 (an extended-precision input keeps its type: the
    finite differences of tests/test_mrf_bwd_truth.py evaluate the forwards in long double)."""
    dt = np.result_type(np.float64, *[np.asarray(a).dtype for a in arrays])
    return [np.asarray(a, dt) for a in arrays]


def sweep_fwd(Sr, rvi, rvc, acc, msgs):
    """One BP sweep: (new messages [n, M], their scatter-add [gx][gy][gz] from zero)."""
    Sr, acc, msgs = _f64(Sr, acc, msgs)
    out = np.zeros(msgs.shape, msgs.dtype)
    acc_out = np.zeros(acc.size, msgs.dtype)
    for r, c, lin in _rays(rvi, rvc, acc.shape):
        out[r, :c] = mb._ray_messages(Sr[r, :c], acc.ravel()[lin], msgs[r, :c])[0]
        np.add.at(acc_out, lin, out[r, :c])
    return out, acc_out.reshape(acc.shape)


def depth_fwd(Sr, rvi, rvc, acc, msgs):
    """The depth distribution [n, M] (zero beyond the count and for skipped rays)."""
    Sr, acc, msgs = _f64(Sr, acc, msgs)
    out = np.zeros(msgs.shape, msgs.dtype)
    for r, c, lin in _rays(rvi, rvc, acc.shape):
        w = mb._ray_messages(Sr[r, :c], acc.ravel()[lin], msgs[r, :c])[1]["w"]
        out[r, :c] = w / w.sum()
    return out


def _bwd(Sr, rvi, rvc, acc, msgs, ray_bwd):
    g_s = np.zeros(msgs.shape)
    g_acc = np.zeros(acc.size)
    g_msgs = np.zeros(msgs.shape)
    for r, c, lin in _rays(rvi, rvc, acc.shape):
        cache = mb._ray_messages(Sr[r, :c], acc.ravel()[lin], msgs[r, :c])[1]
        sbar, mubar = ray_bwd(r, c, lin, Sr[r, :c], cache)
        g_s[r, :c] = sbar
        g_msgs[r, :c] = -mubar
        np.add.at(g_acc, lin, mubar)
    return g_s, g_acc.reshape(acc.shape), g_msgs


def sweep_bwd(Sr, rvi, rvc, acc, msgs, g_msgs_out, g_acc_out=None):
    """(dL/dSr, dL/dacc, dL/dmsgs) of one sweep for dL/d(new messages) = g_msgs_out and
    dL/d(accumulator built from them) = g_acc_out; zero beyond the count and for skipped rays."""
    Sr, acc, msgs, g_msgs_out = _f64(Sr, acc, msgs, g_msgs_out)
    ga = np.zeros(acc.size) if g_acc_out is None else np.asarray(g_acc_out, np.float64).ravel()

    def ray(r, c, lin, s, cache):
        return mb._ray_messages_bwd(g_msgs_out[r, :c] + ga[lin], s, cache)
    return _bwd(Sr, rvi, rvc, acc, msgs, ray)


def depth_bwd(Sr, rvi, rvc, acc, msgs, g_out):
    """The same triple for the depth distribution d = w / W and dL/dd = g_out."""
    Sr, acc, msgs, g_out = _f64(Sr, acc, msgs, g_out)

    def ray(r, c, lin, s, cache):
        W = cache["w"].sum()
        g = g_out[r, :c]
        wbar = (g - (g * cache["w"] / W).sum()) / W
        return mb._chain_from_wbar(wbar, np.zeros(c), np.zeros(c), np.zeros(c), s, cache)
    return _bwd(Sr, rvi, rvc, acc, msgs, ray)


# ------------------------------------------------------------------ fp32 restatement
f32 = np.float32


def _excl_sum_f32(x, reverse=False):
    """lds_excl_sum as one sequential running sum: out[i] = sum_{j<i} x[j] (reverse: j>i)."""
    out = np.empty_like(x)
    run = f32(0)
    for i in (range(len(x) - 1, -1, -1) if reverse else range(len(x))):
        out[i] = run
        run = f32(run + x[i])
    return out, run


def _excl_prod_f32(x):
    out = np.empty_like(x)
    run = f32(1)
    for i in range(len(x)):
        out[i] = run
        run = f32(run * x[i])
    return out


def ray_bwd_fp32(mode, s, a, m, g):
    """k_ray_bwd<mode> on one ray (mode 0: a sweep, 1: the depth distribution) in float32,
    statement by statement.  s, a, m, g: float32 [c] (g already holds g_out + g_acc_next[voxel]).
    Returns (dL/ds, dL/dmu)."""
    assert all(v.dtype == np.float32 for v in (s, a, m, g))
    one, lo, hi = f32(1), f32(1e-4), f32(1 - 1e-4)
    mu = a - m
    e = np.exp(-np.abs(mu))
    sig = np.where(mu > 0, one, e) / (one + e)
    o = np.clip(sig, lo, hi)
    q = one - o
    ds = np.where((sig > lo) & (sig < hi), sig * (one - sig), f32(0))
    T = _excl_prod_f32(q)
    w = o * T * s
    if mode == 0:
        C = _excl_sum_f32(w)[0]
        U = _excl_sum_f32(w, reverse=True)[0]
        pos = C + T * s
        neg = C + U / q
        pbar, nbar = g / pos, -g / neg
        cb = pbar + nbar
        ub = nbar / q
        tb = pbar * s
        sb = pbar * T
        qb = -nbar * U / (q * q)
        wbar = _excl_sum_f32(cb, reverse=True)[0] + _excl_sum_f32(ub)[0]
    else:
        wsum = _excl_sum_f32(w)[1]
        dot = _excl_sum_f32(g * w)[1] / wsum
        wbar = (g - dot) / wsum
        tb = sb = qb = np.zeros_like(s)
    tb = tb + wbar * o * s
    sb = sb + wbar * o * T
    cb = wbar * T * s
    qbar = qb + _excl_sum_f32(tb * T, reverse=True)[0] / q
    mubar = (cb - qbar) * ds
    assert sb.dtype == np.float32 and mubar.dtype == np.float32
    return sb, mubar


def launch_fp32(mode, p):
    """One launch of the restatement on a problem of make_launch: (g_s, g_acc, g_msgs), fp32,
    the accumulator's sums taken in ray order."""
    g_s = np.zeros(p["msgs"].shape, np.float32)
    g_msgs = np.zeros(p["msgs"].shape, np.float32)
    g_acc = np.zeros(p["acc"].size, np.float32)
    for r, c, lin in _rays(p["rvi"], p["rvc"], p["acc"].shape):
        g = p["g_out"][r, :c]
        if mode == 0:
            g = g + p["g_acc_out"].ravel()[lin]
        sb, mubar = ray_bwd_fp32(mode, p["Sr"][r, :c], p["acc"].ravel()[lin], p["msgs"][r, :c], g)
        g_s[r, :c] = sb
        g_msgs[r, :c] = -mubar
        np.add.at(g_acc, lin, mubar)
    return g_s, g_acc.reshape(p["acc"].shape), g_msgs


# ------------------------------------------------------------------ errors
def ray_errors(got, ref, rvc):
    """Per ray: max|got - ref| over the ray's entries / max|ref| over the same entries
    (0 for a ray whose truth is all zero and met exactly)."""
    out = np.zeros(len(rvc))
    for r in range(len(rvc)):
        c = int(rvc[r])
        if c == 0:
            continue
        d = np.abs(np.asarray(got[r, :c], np.float64) - ref[r, :c]).max()
        out[r] = d / np.abs(ref[r, :c]).max() if d > 0 else 0.0
    return out


def launch_error(got, ref):
    d = np.abs(np.asarray(got, np.float64) - ref).max()
    return d / np.abs(ref).max() if d > 0 else 0.0


def output_error(mode, output, regime, got, ref, rvc):
    """The error figure of one output of one launch, on the scale the issue sets for it."""
    if output == "gacc" or (mode, output, regime) in LAUNCH_WIDE:
        return launch_error(got, ref)
    return ray_errors(got, ref, rvc).max()


# ------------------------------------------------------------------ crafted problems
def clip_and_renorm_f32(x):
    """mrf_train.clip_and_renorm on one row, in float32."""
    y = np.clip(x.astype(np.float32), np.float32(1e-5), np.float32(1 - 1e-5))
    return y / y.sum(dtype=np.float32)


def _draw_mu(rng, regime, c):
    if regime == "prior":
        return -3.0 + 0.3 * rng.standard_normal(c)
    if regime == "empty":
        return -6.5 + 0.5 * rng.standard_normal(c)
    mu = 2.0 * rng.standard_normal(c)
    if regime == "saturated":         # a tenth of the entries, rounded down: none in a row of 2 or 3
        sat = rng.permutation(c) < c // 10
        mu = np.where(sat, rng.choice([-1.0, 1.0], c) * (12.0 + 8.0 * rng.random(c)), mu)
    return mu


def _in_band(mu):
    return (np.abs(mu) >= BAND[0]) & (np.abs(mu) <= BAND[1])


def make_launch(counts, M, regime, seed, grid=GRID):
    """A launch of len(counts) rays with exactly these counts (each <= M): fp32 / int32 arrays
    as the kernels take them.  Sr [n, M] clipped + renormalised, rvi [n, M, 3], rvc [n],
    acc [gx][gy][gz], msgs [n, M], g_out [n, M], g_acc_out [gx][gy][gz]."""
    assert regime in REGIMES and max(counts) <= M
    rng = np.random.default_rng(seed)
    n, G = len(counts), int(np.prod(grid))
    rvc = np.asarray(counts, np.int32)
    rvi = np.zeros((n, M, 3), np.int32)
    Sr = np.zeros((n, M), np.float32)
    msgs = np.zeros((n, M), np.float32)
    centre = {"prior": -3.0, "empty": -6.5}.get(regime, 0.0)
    acc = (centre + rng.standard_normal(grid)).astype(np.float32)
    for r, c in enumerate(counts):
        if c == 0:
            continue
        lin = rng.choice(G, c, replace=False)
        rvi[r, :c] = np.stack(np.unravel_index(lin, grid), -1)
        x = rng.random(c) ** 3 + 0.02
        Sr[r, :c] = clip_and_renorm_f32(x / x.sum())
        a = acc.ravel()[lin]
        todo = np.ones(c, bool)
        while todo.any():           # redraw the messages that put mu = acc - msgs into the band
            k = int(todo.sum())
            msgs[r, :c][todo] = (a[todo] - _draw_mu(rng, regime, k)).astype(np.float32)
            todo = _in_band(a - msgs[r, :c]) | _in_band(a.astype(np.float64) - msgs[r, :c])
    p = dict(Sr=Sr, rvi=rvi, rvc=rvc, acc=acc, msgs=msgs, grid=tuple(grid), regime=regime,
             g_out=rng.standard_normal((n, M)).astype(np.float32),
             g_acc_out=rng.standard_normal(grid).astype(np.float32))
    check_launch(p, counts, M)
    return p


@functools.lru_cache(maxsize=None)
def gpu_launch(M, regime):
    """The launch the GPU tests run at this M and regime (shared: do not modify)."""
    return make_launch(GPU_COUNTS[M], M, regime, seed=2000 + M + REGIMES.index(regime))


@functools.lru_cache(maxsize=None)
def gpu_truth(M, regime, mode):
    p = gpu_launch(M, regime)
    if mode == 0:
        return sweep_bwd(p["Sr"], p["rvi"], p["rvc"], p["acc"], p["msgs"], p["g_out"], p["g_acc_out"])
    return depth_bwd(p["Sr"], p["rvi"], p["rvc"], p["acc"], p["msgs"], p["g_out"])


def check_launch(p, counts, M):
    """The conditions every crafted launch meets (conditions on the inputs, not tolerances)."""
    rvi, rvc, grid = p["rvi"], p["rvc"], p["grid"]
    assert rvc.tolist() == list(counts) and rvc.max() <= M and rvi.shape == (len(counts), M, 3)
    assert rvi.min() >= 0 and np.all(rvi < np.asarray(grid, np.int32))
    for r, c in enumerate(counts):
        if c == 0:
            continue
        lin = np.ravel_multi_index(tuple(rvi[r, :c].T.astype(np.int64)), grid)
        assert len(np.unique(lin)) == c
        a = p["acc"].ravel()[lin]
        for mu in (a - p["msgs"][r, :c], a.astype(np.float64) - p["msgs"][r, :c]):
            assert not _in_band(mu).any()
        s = p["Sr"][r, :c]
        assert abs(float(s.sum(dtype=np.float64)) - 1) < 1e-5 and s.min() > 0
