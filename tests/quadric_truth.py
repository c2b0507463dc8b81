"""rn_mesh_place_quadric restated in NumPy (include/raynet_hip.h): every output
vertex of a clustering moved to the minimiser of its summed squared distances to the planes of the
faces around its cluster, the sums in fixed point.  `place_plain` is the definition line by line in
a Python loop (in any order of the faces), `place` the same with np.add.at on int64 and the solve
vectorised over the clusters; both give the bits the kernels have to give.  The meshes of the tests
are here too: the rotated cube, the flat square, the fan and the strips."""
import numpy as np

import simplify_truth as sp

F = np.float32
D = np.float64
I = np.int32
ONE = D(1073741824.0)       # 2^30
REACH = D(2.0)
REGULARIZATION = 2.0 ** -10
MAX_MOVE = 1.0
TERM_BOUND = 3.47           # |term| < 3.47, so |rint(term * 2^30)| < 2^32


def _inputs(vertices, faces, cluster, positions, cell):
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    c = np.asarray(cluster, np.int64).reshape(-1)
    m = np.ascontiguousarray(positions, F).reshape(-1, 3)
    cell = np.broadcast_to(np.asarray(cell, D), (3,)).copy()
    assert len(c) == len(v)
    return v, f, c, m, cell, D(cell.max())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------- the sums
def sums(vertices, faces, cluster, positions, cell):
    """Phases 1 to 3 -> S [nvo, 11] int64: the ten sums and the member count of every output
    vertex."""
    v, f, c, m, cell, L = _inputs(vertices, faces, cluster, positions, cell)
    nv, nvo = len(v), len(m)
    S = np.zeros((nvo, 11), np.int64)
    if nvo == 0:
        return S
    member = (c >= 0) & (c < nvo)
    np.add.at(S[:, 10], c[member], 1)
    f = f[((f >= 0) & (f < nv)).all(1)]
    with np.errstate(all="ignore"):
        p = v[f].astype(D)                                  # [n, corner, axis]
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        ok = np.isfinite(length) & (length > 0)
        f, p, N, length = f[ok], p[ok], N[ok], length[ok]
        n = N / length[:, None]
        share = (0.5 * length) / (L * L)
        w = np.where(share < 1.0, share, 1.0)
        wn = w[:, None] * n
        k = c[f]
        for j in range(3):
            kj = k[:, j]
            use = (kj >= 0) & (kj < nvo)
            for earlier in range(j):
                use &= k[:, earlier] != kj
            r = (p[:, j] - m[np.where(use, kj, 0)].astype(D)) / L
            use &= ((r >= -REACH) & (r <= REACH)).all(1)
            d = -((n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2])
            terms = np.stack([wn[:, 0] * n[:, 0], wn[:, 0] * n[:, 1], wn[:, 0] * n[:, 2],
                              wn[:, 1] * n[:, 1], wn[:, 1] * n[:, 2], wn[:, 2] * n[:, 2],
                              wn[:, 0] * d, wn[:, 1] * d, wn[:, 2] * d, w], 1)[use]
            assert (np.abs(terms) < TERM_BOUND).all()
            np.add.at(S[:, :10], kj[use], np.rint(terms * ONE).astype(np.int64))
    return S


# ------------------------------------------------------------------------------- the solve
def solve(S, positions, cell, regularization=REGULARIZATION, max_move=MAX_MOVE):
    """Phase 4, vectorised over the output vertices -> (positions_out [nvo, 3] float32, counts [2]
    int64, placed [nvo] bool)."""
    m = np.ascontiguousarray(positions, F).reshape(-1, 3)
    cell = np.broadcast_to(np.asarray(cell, D), (3,)).copy()
    L = D(cell.max())
    n = S[:, 10]
    with np.errstate(all="ignore"):
        T = S[:, :10].astype(D) / ONE
        ridge = D(regularization) * T[:, 9]
        m00, m01, m02 = T[:, 0] + ridge, T[:, 1], T[:, 2]
        m11, m12, m22 = T[:, 3] + ridge, T[:, 4], T[:, 5] + ridge
        y0, y1, y2 = -T[:, 6], -T[:, 7], -T[:, 8]
        d0 = m00
        l10, l20 = m01 / d0, m02 / d0
        d1 = m11 - l10 * m01
        e = m12 - l20 * m01
        l21 = e / d1
        d2 = (m22 - l20 * m02) - l21 * e
        z0 = y0
        z1 = y1 - l10 * z0
        z2 = (y2 - l20 * z0) - l21 * z1
        g0, g1, g2 = z0 / d0, z1 / d1, z2 / d2
        x2 = g2
        x1 = g1 - l21 * x2
        x0 = (g0 - l10 * x1) - l20 * x2
        x = np.stack([x0, x1, x2], 1)
        placed = (n > 1) & (S[:, 9] != 0) & (d0 > 0) & (d1 > 0) & (d2 > 0)
        placed &= np.isfinite(l10) & np.isfinite(l20) & np.isfinite(l21) & np.isfinite(x).all(1)
        limit = (D(max_move) * cell) / L
        x = np.where(x > limit, limit, np.where(x < -limit, -limit, x))
        out = (m.astype(D) + L * x).astype(F)
        placed &= np.isfinite(out).all(1)
    result = np.where(placed[:, None], bits(out), bits(m)).view(F)
    moved = placed & (bits(out) != bits(m)).any(1)
    counts = np.array([moved.sum(), (~placed & (n > 1)).sum()], np.int64)
    return result, counts, placed


def place(vertices, faces, cluster, positions, cell, regularization=REGULARIZATION,
          max_move=MAX_MOVE):
    """The definition, vectorised -> (positions_out [nvo, 3] float32, counts [2] int64)."""
    S = sums(vertices, faces, cluster, positions, cell)
    return solve(S, positions, cell, regularization, max_move)[:2]


def place_plain(vertices, faces, cluster, positions, cell, regularization=REGULARIZATION,
                max_move=MAX_MOVE, order=None):
    """The definition line by line, the faces in `order` (any permutation gives the same bits:
    integer sums) -> (positions_out, counts, S)."""
    v, f, c, m, cell, L = _inputs(vertices, faces, cluster, positions, cell)
    nv, nvo = len(v), len(m)
    S = [[0] * 11 for _ in range(nvo)]
    for i in range(nv):
        if 0 <= c[i] < nvo:
            S[c[i]][10] += 1
    with np.errstate(all="ignore"):
        for face in (range(len(f)) if order is None else order):
            i = [int(x) for x in f[face]]
            if not all(0 <= x < nv for x in i):
                continue
            a, b, cc = (v[x].astype(D) for x in i)
            e1, e2 = b - a, cc - a
            N = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                 e1[0] * e2[1] - e1[1] * e2[0]]
            length = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
            if not (np.isfinite(length) and length > 0):
                continue
            n = [N[0] / length, N[1] / length, N[2] / length]
            share = (D(0.5) * length) / (L * L)
            w = share if share < 1.0 else D(1.0)
            wn = [w * n[0], w * n[1], w * n[2]]
            seen = []
            for j in range(3):
                k = int(c[i[j]])
                earlier, seen = k in seen, seen + [k]
                if not 0 <= k < nvo or earlier:
                    continue
                r = (v[i[j]].astype(D) - m[k].astype(D)) / L
                if not ((r >= -REACH) & (r <= REACH)).all():
                    continue
                d = -((n[0] * r[0] + n[1] * r[1]) + n[2] * r[2])
                terms = [wn[0] * n[0], wn[0] * n[1], wn[0] * n[2], wn[1] * n[1], wn[1] * n[2],
                         wn[2] * n[2], wn[0] * d, wn[1] * d, wn[2] * d, w]
                for word, term in enumerate(terms):
                    S[k][word] += int(np.rint(term * ONE))
    S = np.array(S, np.int64).reshape(nvo, 11)
    out, counts, _ = solve(S, m, cell, regularization, max_move)
    return out, counts, S


def simplify_and_place(vertices, faces, cell, regularization=REGULARIZATION, max_move=MAX_MOVE):
    """simplify_truth.simplify on the grid around the vertices, then the placement -> (the four
    arrays of the clustering, positions_out, counts, the grid)."""
    grid = sp.grid_around(vertices, cell)
    mean = sp.simplify(vertices, faces, *grid)
    out, counts = place(vertices, faces, mean[3], mean[0], grid[1], regularization, max_move)
    return mean, out, counts, grid


# ------------------------------------------------------------------------------- the meshes
def cube(n):
    """The unit cube around 0 with n x n quads per side, welded -> (vertices float64, faces)."""
    g = np.linspace(-0.5, 0.5, n + 1)
    V, faces = [], []
    for axis in range(3):
        for side in (-0.5, 0.5):
            base = len(V)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, g[i], g[j]
                    V.append(p)
            for i in range(n):
                for j in range(n):
                    a = base + i * (n + 1) + j
                    b, c, d = a + 1, a + n + 1, a + n + 2
                    faces += [[a, c, b], [b, c, d]] if side > 0 else [[a, b, c], [b, d, c]]
    V, faces = np.array(V, D), np.array(faces, np.int64)
    key = np.round(V * 1e6).astype(np.int64)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return V[first], inverse.reshape(-1)[faces].astype(I)


def rotation():
    a, b = 0.37, 0.61
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return Rz @ Rx


def rotated_cube(n=6):
    """The cube turned by 0.37 about z after 0.61 about x -> (vertices float32, faces int32)."""
    V, faces = cube(n)
    return (V @ rotation().T).astype(F), faces


def cube_distance(points):
    """The distance of points to the surface of the rotated cube, float64."""
    p = np.asarray(points, D) @ rotation()
    q = np.abs(p) - 0.5
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(1))
    inside = np.minimum(q.max(1), 0.0)
    return np.abs(outside + inside)


def flat_square(n=12, z=0.25, side=3.0):
    """A square of n x n quads in the plane z = 0.25, its corner at (0, 0) -> (vertices, faces)."""
    g = (np.arange(n + 1) * (side / n)).astype(F)
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x, y, np.full_like(x, z)], -1).reshape(-1, 3).astype(F)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n + 1, a + 1], 1), np.stack([a + 1, a + n + 1, a + n + 2], 1)])
    return v, f.astype(I)


def fan(nf, seed, radius=0.45):
    """nf faces around a hub, every vertex within `radius` of the hub: with a cell of 1 around the
    hub one cluster takes every face -> (vertices, faces)."""
    rng = np.random.default_rng(seed)
    angle = np.sort(rng.uniform(0.0, 2.0 * np.pi, nf + 1))
    rim = np.stack([np.cos(angle), np.sin(angle), rng.uniform(-0.5, 0.5, nf + 1)], 1)
    rim *= radius * rng.uniform(0.3, 1.0, (nf + 1, 1))
    v = np.concatenate([np.zeros((1, 3)), rim]) + 0.5
    f = np.stack([np.zeros(nf, I), np.arange(1, nf + 1), np.arange(2, nf + 2)], 1)
    return v.astype(F), f.astype(I)


def ridge_strip(nv, seed):
    """A strip of nv vertices along x that zigzags over a ridge (two planes that meet along the x
    axis), pairs of neighbours a quarter apart: with cells of 1 four vertices share a cluster ->
    (vertices, faces)."""
    rng = np.random.default_rng(seed)
    i = np.arange(nv)
    y = np.where(i % 2 == 0, -0.3, 0.3) + rng.uniform(-0.05, 0.05, nv)
    v = np.stack([0.25 * i + rng.uniform(-0.05, 0.05, nv), y, 2.0 - np.abs(y)], 1)
    f = np.stack([i[:-2], i[1:-1], i[2:]], 1)
    return v.astype(F), f.astype(I)


def spread_faces(nf, seed):
    """nf triangles, each in a unit cell of its own along x and a cluster of its own, at the mean
    of its corners moved off the triangle's plane -> (vertices, faces, cluster, positions), the
    clustering written out (the placement takes any `cluster` and any positions)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.1, 0.9, (nf, 3, 3))
    v[:, :, 0] += np.arange(nf)[:, None]
    v = v.astype(F)
    positions = (v.astype(D).mean(1) + rng.uniform(-0.05, 0.05, (nf, 3))).astype(F)
    return (v.reshape(-1, 3), np.arange(3 * nf, dtype=I).reshape(nf, 3),
            np.repeat(np.arange(nf, dtype=I), 3), positions)
