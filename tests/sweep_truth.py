"""Float64 truth of the plane sweep's per-ray prefix -- the plane column (feature_similarities.cu:
66-124), the planes -> voxels map (planes_voxels_mapping.cu:6-92) and the resident path's
clip_and_renorm (mrf_bp.cu:103-111) -- with a forward-error bound per entry, the feature regimes
that make a wrong softmax maximum visible, and the mutants the bound has to reject.  NumPy only.

The INTEGER surfaces are taken as given: `Oracle.feature_indices` (held bit-exact against the
reference's projection and both HIP sweep forms, tests/test_projection_reference.py) says which
feature vector a (ray, view, plane) gathers, `Oracle.plane_indices` which plane pair the monotone
walk gives a voxel.  No entry therefore sits on a rounding boundary the truth could take the other
way, and none is ever excluded from a comparison.

Why regimes.  exp(x - m) / sum exp(x - m) does not depend on m until something over- or
underflows.  Features drawn from N(0, 0.25^2) spread a column's scores over ~0.7: a maximum taken
over the wrong lanes, over one chunk of the planes, or not subtracted at all gives the same
column to rounding.  `peaky` and `extreme` widen the spread within a column, `offset` lifts every
score past exp's overflow, `ramp` sets the scores of neighbouring rays more than exp's underflow
bound apart.

The bound (u = 2^-24, fp32 round to nearest; standard gamma_n terms, first order in u).
  Plane column.  x_k = (1 / P) sum_{pairs} sum_f a_f b_f, P = N (N - 1) / 2, A_k the same with
  absolute values.  F products and F - 1 additions per dot product, P - 1 additions over the
  pairs and one division, in ANY order (the cooperative sweep re-associates, the DPP trees are
  trees), give |fl(x_k) - x_k| <= (F + P) u A_k; one more u covers the resident path's
  multiplication by the rounded 1 / P:                  E_k = (F + P + 1) u A_k.
  d_k = x_k - max x.  The computed maximum is off by at most max_j E_j, the subtraction rounds
  once (u |d_k|), so the exponential's argument is off by E_k + max_j E_j + u |d_k| -- which is
  the RELATIVE error of exp(d_k) -- and the exponential itself adds (2 + 1.5 |d_k|) u: expf is
  good to 1 ulp = 2 u, v_exp_f32 on the rounded product d * log2(e) (the resident path) to
  1.44 |d| u + 1 ulp:        rho_k = E_k + max_j E_j + u |d_k| + (2 + 1.5 |d_k|) u.
  S_k = e_k / sum_j e_j.  The sum's terms carry rho_j each, weighted by S_j; a wave-parallel
  sum of D terms is D / 64 sequential additions per lane and a ceil(log2 D)-deep tree, the
  quotient one division, or a 1-ulp reciprocal and a multiplication (2 u + u), twice at most:
      rel_k = rho_k + sum_j S_j rho_j + (ceil(log2 D) + D / 64 + 2 + 4) u,
      tol_k = S_k rel_k + 1e-37.
  The floor: an exponential below 2^-126 is a denormal (absolute error 2^-150) or flushed to 0
  (error < 1.2e-38), and the column's sum is at least 1 (the maximum's own term).
  Mapped column.  t = clamp(<ray, c - s> / |ray|^2): ray = fl(e - s), c - s, three products, two
  additions, one sum of three squares twice over and a division are 8 roundings at most on terms
  bounded by sum |ray (c - s)| / |ray|^2, the plane positions fl(l * fl(1 / (D - 1))) <= 1 two:
      dt = 8 u sum |ray (c - s)| / |ray|^2 + 2 u.
  c1 = 1 - left_d / (left_d + right_d) moves by at most 2 dt / (left_d + right_d) and rounds four
  times on values <= 1 (a hardware reciprocal there, 1 ulp = 2 u on a quotient <= 1, adds 2 u:
  `reciprocal`):                 dc = 2 dt / (left_d + right_d) + 4 u  (+ 2 u).
  val = c1 S[l] + c2 S[l + 1] (two products, one addition, and the inputs' own tolerance):
      tol_val = |c1| tolS[l] + |c2| tolS[l + 1] + dc (|S[l]| + |S[l + 1]|) + 4 u |val|,
  Sv = val / sum val, the sum over `count` terms as above:
      tol_Sv = tol_val / sum + Sv (sum tol_val / sum + (log2 count + count / 64 + 3) u)
  (`reciprocal`: the quotient is a 1-ulp reciprocal and a product, 3 u where the division has 1:
  + 2 u).
  Resident column.  The clamp to [1e-5, 1 - 1e-5] is 1-Lipschitz: tol + u y; then the same sum
  and quotient terms once more.
"""
import collections
import math

import numpy as np

from conftest import load_cases

U = 2.0 ** -24
FLOOR = 1e-37
CLIP_LO, CLIP_HI = np.float32(1e-5), np.float32(1 - 1e-5)
REGIMES = ("flat", "peaky", "extreme", "offset", "ramp", "constant", "zero")
# generator constants (part of the cases: the CPU tests assert what each has to achieve)
# extreme: at 4.0 the 36-pair mean of a 9-view case spreads a column over 93 only, and no column's
# maximum lies 88.7 above its first 64 planes; at 6.0 every case is beyond exp's underflow bound
# (103.28) and the D = 128 / 129 cases show a maximum taken over the first chunk of planes
SIGMA = {"flat": 0.25, "peaky": 1.5, "extreme": 6.0}
OFFSET_C = 10.0          # c^2 = 100: every score of `offset` is lifted by 100 > ln(FLT_MAX) = 88.7
RAMP_SLOPE = 0.5         # channel value per feature-map row: see ramp_channel

CU = load_cases("crosscheck_cu_host.npz")
F_OF = {"wide": 32, "aniso": 16, "small": 8}

Case = collections.namedtuple("Case", "geometry D N F padding regime n")
Case.__new__.__defaults__ = (61,)


def case_id(c):
    return "%s-D%d-N%d-F%d-p%d-%s-n%d" % c


# ------------------------------------------------------------------ cases
def views(geometry, D, N):
    """[N, 3, 4] cameras: the fixture's, and beyond them the fixture's with slightly different
    matrices (as test_packed_sweep_gpu._case makes them)."""
    P = np.array(CU[geometry]["P"], np.float32)
    rng = np.random.default_rng(1000 * D + N)
    while len(P) < N:
        P = np.concatenate([P, P[1:] * (1 + 0.01 * rng.standard_normal(P[1:].shape)).astype(np.float32)])
    return np.ascontiguousarray(P[:N])


def features(case, shape):
    """[N, H + padding + 1, W + padding + 1, F] float32 of the case's regime, seeded by the shape."""
    g, D, N, F, padding, regime, n = case
    rng = np.random.default_rng([REGIMES.index(regime), D, N, F, padding])
    if regime == "constant":
        return np.full(shape, 0.5, np.float32)
    if regime == "zero":
        f = np.zeros(shape, np.float32)
        f[rng.random(shape) < 0.3] = -0.0
        return f
    sigma = SIGMA.get(regime, SIGMA["flat"])
    f = rng.standard_normal(shape, dtype=np.float32) * np.float32(sigma)
    if regime == "offset":
        f[..., F // 2] = np.float32(OFFSET_C)
    if regime == "ramp":
        f[..., F // 2] = ramp_channel(shape[1])[None, :, None]
    return f


def ramp_channel(Hf):
    """One channel that grows with the feature map's ROW.  A pair of views that sees a point in rows
    a and b scores RAMP_SLOPE^2 a b from it.  The fixtures' views sit side by side: along a ray a
    point's row barely moves in any view (a column's scores stay within ~30 of each other, every
    plane above fp32's underflow) while its column crosses the image (a ramp along the columns
    spreads a column's own scores 2 - 5 times wider than it sets neighbouring rays apart, and the
    fp32 map of such a column is 0 / 0 in the reference itself).  Consecutive rays of the fixtures'
    lists lie in different rows: the maxima of most groups of 2 / 4 are more than 104 apart, exp's
    whole fp32 range."""
    return (np.float32(RAMP_SLOPE) * np.arange(Hf, dtype=np.float32)).astype(np.float32)


# Every ray of the fixtures enters its grid.  Rays with no voxel or one (what the resident path
# never reads) are pixels beyond the image's last column, whose rays pass the box: one next to live
# rays in its wavefront, one whole wavefront of four, one next to a live ray in a wavefront of
# two, and the last ray of the launch, alone in its wavefront.  7 of 61.
SHORT_SLOTS = (1, 8, 9, 10, 11, 30, 60)
_GEOMETRY = {}


def rays(o, geometry, n):
    """The first n rays of the fixture; for n = 61 with SHORT_SLOTS replaced by rays of 0 and of 1
    voxels, alternately."""
    c = CU[geometry]
    ridx = np.array(c["ray_idxs"], np.int32)[:n].copy()
    assert len(ridx) == n
    if n > max(SHORT_SLOTS):
        beyond = np.arange(o.H * o.W, 5 * o.H * o.W, dtype=np.int32)
        s, e = o.sample(beyond, c["P_inv"], c["center"])
        cnt = o.traversal(s, e)[1]
        short = [beyond[cnt == 0][0], beyond[cnt == 1][0]]
        for k, slot in enumerate(SHORT_SLOTS):
            ridx[slot] = short[k % 2]
    return np.ascontiguousarray(ridx)


class Built(object):
    """One case made concrete: oracle, cameras, features, rays, and the integer surfaces."""


def build(oracle_mod, case):
    g, D, N, F, padding, regime, n = case
    c = CU[g]
    assert F == F_OF[g]
    key = (g, D, N, padding, n)
    geo = _GEOMETRY.get(key)
    if geo is None:                     # shared by the regimes of a shape: ~70 k ctypes calls
        geo = Built()
        geo.o = o = oracle_mod.Oracle(M=int(c["M"]), D=D, N=N, F=F, H=int(c["H"]), W=int(c["W"]),
                                      padding=padding, bbox=c["bbox"], grid_shape=c["grid"])
        geo.P = views(g, D, N)
        geo.P_inv, geo.center = np.array(c["P_inv"], np.float32), np.array(c["center"], np.float32)
        geo.ridx = rays(o, g, n)
        geo.starts, geo.ends = o.sample(geo.ridx, geo.P_inv, geo.center)
        geo.idx = o.feature_indices(geo.P, geo.starts, geo.ends)
        geo.vg = oracle_mod.voxel_grid_centers(c["bbox"], c["grid"])
        geo.rvi, geo.rvc = o.traversal(geo.starts, geo.ends)
        geo.left = o.plane_indices(geo.vg, geo.rvi, geo.rvc, geo.starts, geo.ends)
        _GEOMETRY[key] = geo
    b = Built()
    b.__dict__.update(geo.__dict__)
    b.case = case
    b.feats = features(case, (N, b.o.H + padding + 1, b.o.W + padding + 1, F))
    return b


def centres(b, r):
    """[count, 3] float32 voxel centres of ray r."""
    v = b.rvi[r, :b.rvc[r]]
    return b.vg[v[:, 0], v[:, 1], v[:, 2]]


# ------------------------------------------------------------------ the truth
def scores(features, idx, drop_pair=False):
    """x [n, D] and A [n, D] in float64: the pair sums of the F-term dot products and of their
    absolute values, NOT yet divided by the pair count.  drop_pair: without the last pair."""
    n, N, D, _ = idx.shape
    f = features.astype(np.float64)
    g = f[np.arange(N)[None, :, None], idx[..., 1], idx[..., 0]]            # [n, N, D, F]
    x = np.zeros((n, D))
    A = np.zeros((n, D))
    pairs = [(i, j) for i in range(N) for j in range(i + 1, N)]
    for i, j in pairs[:len(pairs) - 1 if drop_pair else None]:
        pr = g[:, i] * g[:, j]
        x += pr.sum(-1)
        A += np.abs(pr).sum(-1)
    return x, A, len(pairs)


def softmax64(x):
    d = x - x.max(-1, keepdims=True)
    e = np.exp(d)
    return e / e.sum(-1, keepdims=True), d


def column_truth(features, idx, F):
    """(S64 [n, D], tol [n, D]) of the plane column; see the module's docstring for the bound."""
    assert features.shape[-1] == F
    x, A, P = scores(features, idx)
    x, A = x / P, A / P
    D = x.shape[1]
    S, d = softmax64(x)
    E = (F + P + 1) * U * A
    rho = E + E.max(-1, keepdims=True) + U * np.abs(d) + (2 + 1.5 * np.abs(d)) * U
    rel = rho + (S * rho).sum(-1, keepdims=True) + (math.ceil(math.log2(D)) + D / 64.0 + 2 + 4) * U
    return S, S * rel + FLOOR


def voxel_truth(S64, tolS, left, centres, start, end, count, D, reciprocal=False):
    """One ray: (Sv64 [count], tol [count]).  S64, tolS [D]; left [>= count] the walk's own plane
    index per voxel; centres [count, 3], start / end [3] float32.  reciprocal: the value-only
    quotients go through a 1-ulp hardware reciprocal (the resident path)."""
    assert count >= 1
    s, e = np.asarray(start, np.float64), np.asarray(end, np.float64)
    c = np.asarray(centres, np.float64)[:count]
    left = np.asarray(left[:count], np.int64)
    assert left.min() >= 0 and left.max() + 1 <= D - 1
    ray = e - s
    norm = (ray * ray).sum()
    prod = ray[None, :] * (c - s[None, :])
    t = np.clip(prod.sum(1) / norm, 1e-4, 1 - 1e-4)
    step = 1.0 / (D - 1)
    left_d, right_d = np.abs(t - left * step), np.abs(t - (left + 1) * step)
    c1, c2 = 1 - left_d / (left_d + right_d), 1 - right_d / (left_d + right_d)
    Sl, Sr = S64[left], S64[left + 1]
    val = c1 * Sl + c2 * Sr
    tot = val.sum()
    Sv = val / tot
    dt = 8 * U * np.abs(prod).sum(1) / norm + 2 * U
    dc = 2 * dt / (left_d + right_d) + (6 if reciprocal else 4) * U
    tol_val = np.abs(c1) * tolS[left] + np.abs(c2) * tolS[left + 1] + dc * (np.abs(Sl) + np.abs(Sr)) \
        + 4 * U * np.abs(val)
    quot = (math.log2(count) + count / 64.0 + (5 if reciprocal else 3)) * U
    return Sv, tol_val / tot + Sv * (tol_val.sum() / tot + quot)


def resident_truth(Sv64, tol):
    """clip_and_renorm of one ray's mapped column: (Sr64, tol)."""
    count = len(Sv64)
    y = np.clip(Sv64, float(CLIP_LO), float(CLIP_HI))
    ty = tol + U * y
    tot = y.sum()
    Sr = y / tot
    return Sr, ty / tot + Sr * (ty.sum() / tot + (math.log2(count) + count / 64.0 + 5) * U)


def truths(b, chained=True, reciprocal=False, column=None):
    """Everything for a built case: S64, tolS [n, D]; per ray Sv, tolv and Sr, tolr (lists; None for
    a ray without voxels).  chained: the map's input is the plane column's truth with ITS tolerance
    (the sweep's own tail); otherwise the truth rounded to fp32, tolS = u S + 1e-37 (K6 fed with it).
    column: column_truth's answer, when the caller has it."""
    S, tolS = column if column is not None else column_truth(b.feats, b.idx, b.o.F)
    # (rounding to fp32 is u S down to 2^-126 only: below, a denormal is 2^-150 off and a launch
    # may flush it to 0 -- the column's own floor)
    Sin, tin = (S, tolS) if chained else (S.astype(np.float32).astype(np.float64), U * S + FLOOR)
    Sv, tv, Sr, tr = [], [], [], []
    for r in range(len(b.ridx)):
        cnt = int(b.rvc[r])
        if cnt < 1:
            Sv.append(None), tv.append(None), Sr.append(None), tr.append(None)
            continue
        a, ta = voxel_truth(Sin[r], tin[r], b.left[r], centres(b, r), b.starts[r], b.ends[r], cnt,
                            b.o.D, reciprocal)
        Sv.append(a), tv.append(ta)
        a, ta = resident_truth(a, ta)
        Sr.append(a), tr.append(ta)
    return S, tolS, Sv, tv, Sr, tr


def worst_ratio(got, truth, tol):
    """max |got - truth| / tol over EVERY entry; a non-finite entry counts as infinitely wrong."""
    got = np.asarray(got, np.float64)
    r = np.abs(got - truth) / tol
    r[~np.isfinite(got)] = np.inf
    return float(r.max())


def unpack_voxels(vox):
    """packed ids (x << 20 | y << 10 | z) -> [..., 3]"""
    vox = np.asarray(vox)
    return np.stack([vox >> 20, (vox >> 10) & 1023, vox & 1023], -1).astype(np.int32)


# ------------------------------------------------------------------ mutants
def _softmax32(x32, mx, sum_over=None, extra=0.0):
    """fp32 exp(x - mx) / sum, the way a kernel would: overflow to inf, underflow to 0."""
    with np.errstate(all="ignore"):
        e = np.exp((x32 - mx).astype(np.float32)).astype(np.float32)
        tot = (e if sum_over is None else e[:, :sum_over]).sum(-1, keepdims=True, dtype=np.float32)
        return (e / (tot + np.float32(extra))).astype(np.float32)


def _x32(b, drop_pair=False, divide_by=None):
    x, _, P = scores(b.feats, b.idx, drop_pair)
    return (x / (divide_by or P)).astype(np.float32)


def column_plain(b):
    """The unmutated fp32 column (the mutants' control)."""
    x = _x32(b)
    return _softmax32(x, x.max(-1, keepdims=True))


def mutant_neighbour_max(b, group):
    """1: the maximum over each group of 2 / 4 consecutive rays (the rays that share a packed
    wavefront) used for every ray of the group."""
    x = _x32(b)
    mx = x.max(-1, keepdims=True).copy()
    for r0 in range(0, len(mx), group):
        mx[r0:r0 + group] = mx[r0:r0 + group].max()
    return _softmax32(x, mx)


def mutant_no_max(b):
    """2: no maximum subtracted."""
    return _softmax32(_x32(b), np.float32(0))


def mutant_first_chunk(b, chunk=64):
    """3: for D > 64 the maximum and the sum over the first 64 planes only."""
    x = _x32(b)
    return _softmax32(x, x[:, :chunk].max(-1, keepdims=True), sum_over=chunk)


def mutant_first_chunk_max(b, chunk=64):
    """3b: the maximum over the first 64 planes only, the sum over all of them -- shift invariance
    hides it until exp(x - m) overflows: a spread beyond 88.7 with the maximum past plane 63."""
    x = _x32(b)
    return _softmax32(x, x[:, :chunk].max(-1, keepdims=True))


def mutant_pair_dropped(b):
    """4: one pair dropped from the mean."""
    x = _x32(b, drop_pair=True)
    return _softmax32(x, x.max(-1, keepdims=True))


def mutant_pair_count(b):
    """5: division by N (N - 1) instead of the pair count."""
    x = _x32(b, divide_by=b.o.N * (b.o.N - 1))
    return _softmax32(x, x.max(-1, keepdims=True))


def mutant_rolled(b):
    """6: the column rolled by one plane."""
    return np.roll(column_plain(b), 1, axis=1)


def mutant_padding_counted(b):
    """7: planes >= D of a padded group (16, 32 or a multiple of 64 lanes) counted in the sum as
    exp(0)."""
    D = b.o.D
    pad = (16 if D <= 16 else 32 if D <= 32 else -(-D // 64) * 64) - D
    x = _x32(b)
    return _softmax32(x, x.max(-1, keepdims=True), extra=float(pad))


def _map32(b, S, right_clamp=None, over_M=False):
    """fp32-shaped planes -> voxels from a column S [n, D] (float64 arithmetic, cast at the end);
    [n, M], zero beyond count."""
    D, M = b.o.D, b.o.M
    out = np.zeros((len(b.ridx), M), np.float32)
    step = 1.0 / (D - 1)
    for r in range(len(b.ridx)):
        cnt = int(b.rvc[r])
        if cnt < 1:
            continue
        m = M if over_M else cnt            # (9: the rows' zero tail = voxel (0, 0, 0), walk held)
        v = b.rvi[r, :m]
        c = b.vg[v[:, 0], v[:, 1], v[:, 2]].astype(np.float64)
        s, e = b.starts[r].astype(np.float64), b.ends[r].astype(np.float64)
        ray = e - s
        t = np.clip((ray * (c - s)).sum(1) / (ray * ray).sum(), 1e-4, 1 - 1e-4)
        left = np.concatenate([b.left[r, :cnt], np.full(m - cnt, b.left[r, cnt - 1])]).astype(np.int64)
        right = left + 1 if right_clamp is None else np.minimum(left + 1, right_clamp)
        ld, rd = np.abs(t - left * step), np.abs(t - (left + 1) * step)
        val = (1 - ld / (ld + rd)) * S[r][left] + (1 - rd / (ld + rd)) * S[r][right]
        out[r, :cnt] = (val / val.sum())[:cnt]
    return out


def mapped_plain(b, S):
    return _map32(b, S)


def mutant_right_clamped(b, S):
    """8: `left + 1` clamped one short at the last plane."""
    return _map32(b, S, right_clamp=b.o.D - 2)


def mutant_sum_over_M(b, S):
    """9: the normaliser summed over M instead of count."""
    return _map32(b, S, over_M=True)


# ------------------------------------------------------------------ shapes of the launch tests
# (flavour, geometry, D, N, padding, options): the smallest shapes at which each flavour's edges
# occur -- D at both ends of a packing and one inside, D past one and two chunks of 64 planes,
# 2 .. 10 views, F = 8 / 16 / 32, odd and even padding
SHAPES = [
    ("packed4", "wide", 2, 5, 11, {}), ("packed4", "wide", 9, 9, 11, {}), ("packed4", "wide", 16, 3, 11, {}),
    ("packed2", "wide", 17, 2, 11, {}), ("packed2", "wide", 27, 9, 11, {}), ("packed2", "wide", 32, 5, 11, {}),
    ("coop", "wide", 16, 3, 11, {"sweep_rays_per_wave": 1}), ("coop", "wide", 32, 5, 11, {"sweep_rays_per_wave": 1}),
    ("coop", "wide", 33, 4, 11, {}), ("coop", "wide", 64, 5, 11, {}), ("coop", "wide", 65, 2, 11, {}),
    ("coop", "wide", 100, 9, 11, {}), ("coop", "wide", 128, 6, 11, {}), ("coop", "wide", 129, 7, 11, {}),
    ("generic", "wide", 32, 5, 11, {"generic_sweep": True}), ("generic", "wide", 100, 9, 11, {"generic_sweep": True}),
    ("generic", "aniso", 33, 4, 11, {}), ("generic", "small", 16, 3, 5, {}), ("generic", "wide", 64, 10, 11, {}),
    ("coop-even", "wide", 64, 5, 10, {}), ("generic-even", "wide", 64, 5, 10, {"generic_sweep": True}),
]
# extreme / constant / zero (and n = 1) run on one shape per flavour
RARE_SHAPE = {"packed4": 9, "packed2": 27, "coop": 128, "generic": 100, "coop-even": 64, "generic-even": 64}
EVERY, RARE = ("flat", "peaky", "offset", "ramp"), ("extreme", "constant", "zero")


def launch_cases():
    """[(flavour, options, Case)] of tests/test_sweep_launches_gpu.py."""
    out = []
    for flavour, g, D, N, padding, opts in SHAPES:
        rare = RARE_SHAPE[flavour] == D and g == "wide" and N != 10
        for regime in EVERY + (RARE if rare else ()):
            out.append((flavour, opts, Case(g, D, N, F_OF[g], padding, regime)))
        if rare and not flavour.endswith("even"):
            out.append((flavour, opts, Case(g, D, N, F_OF[g], padding, "peaky", 1)))
    return out
