"""NumPy restatements of the evaluation kernels of csrc/raynet_eval.inl,
operation for operation in the kernels' order: the library is built with -ffp-contract=off, so
every +, -, *, / and sqrt below is the one correctly rounded operation the kernel does and the
results are the kernels' bits.  No GPU, no torch.

    depth_points      k_depth_points     back-projection of a depth map, float64
    consistency_tau   k_consistency_tau  one neighbour view of the consistency check, float64
    nearest           k_nn               exact nearest neighbour on float32 rows [n][4]

and the clouds the CPU and the GPU tests share (lattice_cloud, dtu_cloud).
"""
import numpy as np

F32 = np.float32
NN_TILE = 2048          # reference points per LDS tile of k_nn
NN_BLOCK = 256          # lanes per workgroup; every lane holds NN_Q = 2 queries


def depth_points(H, W, P_pinv, center, depth):
    """(3, H*W) float64: the point of pixel i = u*H + v at column i.  P_pinv [4][3], center [4]
    (all four components enter the norm), depth (H, W) float32."""
    P = np.asarray(P_pinv, np.float64).reshape(12)
    c = np.asarray(center, np.float64).reshape(4)
    depth = np.asarray(depth)
    assert depth.shape == (H, W) and depth.dtype == F32
    i = np.arange(H * W)
    ui, vi = i // H, i % H
    u, v = ui.astype(np.float64), vi.astype(np.float64)
    with np.errstate(all="ignore"):
        r = [(P[3 * k] * u + P[3 * k + 1] * v) + P[3 * k + 2] * 1.0 for k in range(4)]
        d = [r[k] / r[3] - c[k] for k in range(4)]
        norm = np.zeros(H * W)
        for k in range(4):
            norm = norm + d[k] * d[k]
        norm = np.sqrt(norm)
        t = depth[vi, ui].astype(np.float64)
        return np.stack([c[k] + (t * d[k]) / norm for k in range(3)])


def projection(points, P):
    """The doubles k_consistency_tau rounds: (h0 / h2, h1 / h2) of points (3, n) under P [3][4]."""
    x, y, z = (np.asarray(points, np.float64)[k] for k in range(3))
    P = np.asarray(P, np.float64).reshape(12)
    with np.errstate(all="ignore"):
        h = [((P[4 * k] * x + P[4 * k + 1] * y) + P[4 * k + 2] * z) + P[4 * k + 3] * 1.0
             for k in range(3)]
        return h[0] / h[2], h[1] / h[2]


def consistency_tau(points, P, center, depth, tau_in, first):
    """float64 [n]: tau after one neighbour view.  points (3, n), P [3][4], center [4], depth
    (H, W) float32 (raw: NaN stays NaN), tau_in [n] (not read when `first`)."""
    points = np.asarray(points, np.float64)
    c = np.asarray(center, np.float64).reshape(4)
    depth = np.asarray(depth)
    assert depth.ndim == 2 and depth.dtype == F32
    H, W = depth.shape
    n = points.shape[1]
    qx, qy = projection(points, P)
    with np.errstate(all="ignore"):
        X, Y = np.rint(qx), np.rint(qy)                 # half to even
        # decided on the doubles: NaN and +-inf fail every comparison they must fail
        valid = (0 <= X) & (X < W) & (0 <= Y) & (Y < H)
        xi = np.where(valid, X, 0.0).astype(np.int64)
        yi = np.where(valid, Y, 0.0).astype(np.int64)
        predicted = depth[yi, xi].astype(np.float64)
        p = [points[0], points[1], points[2], np.ones(n)]
        dist = np.zeros(n)
        for k in range(4):
            e = p[k] - c[k]
            dist = dist + e * e
        dist = np.sqrt(dist)
        diff = np.abs(predicted - dist)
        t = diff if first else np.maximum(diff, np.asarray(tau_in, np.float64)[:n])
        return np.where(valid, t, np.inf)


def nearest(ref_xyzw, query_xyzw, chunk=512):
    """(dist float32 [nq], idx int32 [nq]) of the scan over float32 rows [n][4]: idx is the lowest
    index whose d2 is strictly below every earlier one (a NaN d2 is below nothing, an inf d2 is
    not below the starting inf), -1 and dist = inf if there is none.  Column 3 is never read."""
    ref = np.asarray(ref_xyzw)
    qry = np.asarray(query_xyzw)
    assert ref.dtype == F32 and qry.dtype == F32 and ref.shape[1:] == (4,) and qry.shape[1:] == (4,)
    nq = qry.shape[0]
    dist = np.full(nq, np.inf, F32)
    idx = np.full(nq, -1, np.int32)
    if ref.shape[0] == 0:
        return dist, idx
    with np.errstate(all="ignore"):
        for s in range(0, nq, chunk):
            q = qry[s:s + chunk]
            dx = q[:, None, 0] - ref[None, :, 0]
            dy = q[:, None, 1] - ref[None, :, 1]
            dz = q[:, None, 2] - ref[None, :, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            d2 = np.where(np.isnan(d2), F32(np.inf), d2)
            first = d2.argmin(axis=1)                       # the first of equal minima
            best = d2[np.arange(len(q)), first]
            found = best < np.inf
            idx[s:s + chunk] = np.where(found, first, -1)
            dist[s:s + chunk] = np.sqrt(best)
    assert dist.dtype == F32
    return dist, idx


def squared_distances(ref_xyzw, query_xyzw):
    """The float32 d2 of every (query, reference) pair, [nq][n_ref] -- for the tests' premises."""
    ref, qry = np.asarray(ref_xyzw), np.asarray(query_xyzw)
    dx = qry[:, None, 0] - ref[None, :, 0]
    dy = qry[:, None, 1] - ref[None, :, 1]
    dz = qry[:, None, 2] - ref[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == F32
    return d2


def xyzw(xyz, w=0.0):
    """(n, 3) -> [n][4] float32 rows with `w` in the unused lane."""
    xyz = np.asarray(xyz)
    out = np.full((xyz.shape[0], 4), w, F32)
    out[:, :3] = xyz
    return out


def lattice_cloud(n_ref, n_query, seed=0):
    """Reference rows with integer coordinates in 0..5 (216 sites: ties as soon as n_ref exceeds a
    few hundred, exact duplicates among them), queries at integers plus 0 or 0.5: every d2 is a
    multiple of 0.25 below 2^7, exact in float32, and equal distances are equal bits."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 6, (n_ref, 3)).astype(F32)
    qry = (rng.integers(0, 6, (n_query, 3)) + 0.5 * rng.integers(0, 2, (n_query, 3))).astype(F32)
    return xyzw(ref), xyzw(qry)


def dtu_cloud(n_ref, n_query, seed=0):
    """Coordinates at DTU scale: reference points uniform in [300, 700)^3, every query 0.2 away
    from a reference point in a random direction."""
    rng = np.random.default_rng(seed)
    ref = (rng.random((n_ref, 3)) * 400 + 300).astype(F32)
    step = rng.standard_normal((n_query, 3))
    step *= 0.2 / np.linalg.norm(step, axis=1, keepdims=True)
    qry = (ref[rng.integers(0, n_ref, n_query)].astype(np.float64) + step).astype(F32)
    return xyzw(ref), xyzw(qry)


def same_bits(a, b):
    """Equal shapes and dtypes, NaN at the same places (a NaN's payload and sign are not part of
    any contract here), every other element equal bit for bit (so -0.0 is not 0.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(np.ascontiguousarray(a)[~na].view(bits),
                               np.ascontiguousarray(b)[~nb].view(bits)))
