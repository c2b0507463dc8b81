"""Which views see a point, how many points two views share, and what a greedy covering set
picks, restated in NumPy (include/raynet_hip.h: rn_view_overlap /
rn_view_gain): the definition the GPU tests hold the kernels to integer for integer.

Everything is np.float64 arithmetic, one ufunc per operation and in the definition's order (NumPy
fuses nothing), vectorised over the points per view and per pair of views; the counts are integer
sums.  The projection is appearance_truth.project_points.  Nothing here is taken from the kernels.

`mutant` names one deliberate mistake, for the tests that show that their cases tell it from the
definition: "band_on_c" (the squares compared with c q instead of c c q),
"one_sees" (a pair counted when only one of its views sees the point), "chosen_ignored" (the short
test without `chosen`).
"""
import numpy as np

from appearance_truth import PlaneCamera, pack_cameras, project_points  # noqa: F401

F = np.float32
D = np.float64
U = np.uint64
MAX_VIEWS = 64


def low_bits(V):
    return U(0xFFFFFFFFFFFFFFFF) if V >= 64 else U((1 << V) - 1)


def popcount(mask):
    """The number of set bits of every uint64 of `mask`, as int64."""
    m = np.ascontiguousarray(mask, U)
    return np.unpackbits(m.view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(-1, dtype=np.int64)


def bit(mask, v):
    """[n] bool: bit v of every uint64."""
    return ((np.asarray(mask, U) >> U(v)) & U(1)).astype(bool)


def visible(points, normals, cameras, image_shape, depths, tol, min_cos, border):
    """points [n, 3] f64, normals [n, 3] f64 or None, cameras [V, 15] f64, image_shape (H, W),
    depths [V, H, W] f32 or None -> [n] uint64, bit v set iff view v sees the point."""
    p = np.asarray(points, D).reshape(-1, 3)
    nr = np.zeros_like(p) if normals is None else np.asarray(normals, D).reshape(-1, 3)
    cameras = np.asarray(cameras, D).reshape(-1, 15)
    V = len(cameras)
    H, W = image_shape
    assert 1 <= V <= MAX_VIEWS and len(nr) == len(p)
    tol, min_cos, border = D(tol), D(min_cos), D(border)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    mask = np.zeros(len(p), U)
    with np.errstate(all="ignore"):
        nx, ny, nz = nr[:, 0], nr[:, 1], nr[:, 2]
        nn = (nx * nx + ny * ny) + nz * nz
        facing = nn > 0
        mc2 = min_cos * min_cos
        x_max, y_max = D(W - 1) - border, D(H - 1) - border
        for v in range(V):
            X, Y, dx, dy, dz, dd, ok = project_points(cameras[v], x, y, z, border, x_max, y_max)
            dot = (nx * dx + ny * dy) + nz * dz
            q = nn * dd
            dot2 = dot * dot
            ok = ok & (~facing | ((dot > 0) & (dot2 > mc2 * q)))
            if depths is not None:
                Xs, Ys = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
                zf = np.asarray(depths, F)[v][np.rint(Ys).astype(np.int64),
                                              np.rint(Xs).astype(np.int64)]
                lim = zf.astype(D) + tol
                ok = ok & (zf > 0) & (dd <= lim * lim)
            mask = np.where(ok, mask | (U(1) << U(v)), mask).astype(U)
    return mask


def pair_counts(points, mask, cameras, cos_lo, cos_hi, mutant=None):
    """[V, V] int64: on the diagonal the number of points every view sees, above it the number of
    points the two views share; the lower triangle is 0."""
    p = np.asarray(points, D).reshape(-1, 3)
    cameras = np.asarray(cameras, D).reshape(-1, 15)
    V = len(cameras)
    cos_lo, cos_hi = D(cos_lo), D(cos_hi)
    assert 0 <= cos_lo <= cos_hi <= 1
    lo2, hi2 = cos_lo * cos_lo, cos_hi * cos_hi
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    pairs = np.zeros((V, V), np.int64)
    with np.errstate(all="ignore"):
        d = [(cameras[v, 12] - x, cameras[v, 13] - y, cameras[v, 14] - z) for v in range(V)]
        dd = [(a * a + b * b) + c * c for a, b, c in d]
        for i in range(V):
            si = bit(mask, i)
            pairs[i, i] = int(si.sum())
            for j in range(i + 1, V):
                sj = bit(mask, j)
                both = (si | sj) if mutant == "one_sees" else (si & sj)
                dot = (d[i][0] * d[j][0] + d[i][1] * d[j][1]) + d[i][2] * d[j][2]
                q = dd[i] * dd[j]
                dot2 = dot * dot
                if mutant == "band_on_c":
                    band = (dot > 0) & (dot2 >= cos_lo * q) & (dot2 <= cos_hi * q)
                else:
                    band = (dot > 0) & (dot2 >= lo2 * q) & (dot2 <= hi2 * q)
                pairs[i, j] = int((both & band).sum())
    return pairs


def view_overlap(points, normals, cameras, image_shape, depths, tol, min_cos, border, cos_lo,
                 cos_hi, mutant=None):
    """rn_view_overlap on zeroed pairs -> (visible [n] uint64, pairs [V, V] int64)."""
    mask = visible(points, normals, cameras, image_shape, depths, tol, min_cos, border)
    return mask, pair_counts(points, mask, cameras, cos_lo, cos_hi, mutant)


def gain(mask, V, chosen, redundancy, mutant=None):
    """rn_view_gain on a zeroed gain -> [V + 1] int64.  chosen: a Python int, the 64-bit mask."""
    mask = np.asarray(mask, U)
    assert 1 <= V <= MAX_VIEWS and 1 <= redundancy <= 64
    chosen = U(int(chosen) & 0xFFFFFFFFFFFFFFFF)
    taken = low_bits(V) if mutant == "chosen_ignored" else (chosen & low_bits(V))
    short = popcount(mask & taken) < redundancy
    out = np.zeros(V + 1, np.int64)
    for v in range(V):
        if not (int(chosen) >> v) & 1:
            out[v] = int((short & bit(mask, v)).sum())
    out[V] = int(short.sum())
    return out


def symmetric(pairs):
    """The matrix mirrored: what ViewOverlap.pairs holds."""
    pairs = np.asarray(pairs, np.int64)
    return np.triu(pairs) + np.triu(pairs, 1).T


def neighbors(pairs, i, k):
    """The k views j != i with the largest pairs[i, j] of the symmetric matrix: ties to the lower
    j, views that share nothing last, in index order."""
    row = [(-int(pairs[i, j]), j) for j in range(len(pairs)) if j != i]
    return [j for _, j in sorted(row)][:k]


def cover(mask, V, k, redundancy=1, candidates=None, mutant=None):
    """The greedy covering set -> (order, gains, short): the views in the order chosen, the gain
    each had when chosen, and the number of points still short at the end."""
    allowed = range(V) if candidates is None else sorted(set(int(c) for c in candidates))
    chosen, order, gains = 0, [], []
    while len(order) < k:
        g = gain(mask, V, chosen, redundancy, mutant)
        best, best_gain = -1, 0
        for v in allowed:
            if not (chosen >> v) & 1 and g[v] > best_gain:
                best, best_gain = v, int(g[v])
        if best < 0:
            break
        order.append(best)
        gains.append(best_gain)
        chosen |= 1 << best
    return order, gains, int(gain(mask, V, chosen, redundancy, mutant)[V])


# ------------------------------------------------------------------------------- the inputs
def ring_scene(V=8, radius=1.5, height=3.0, focal=20.0, H=24, W=32, side=41, extent=2.5):
    """V PlaneCameras on a ring over the plane z = 0 and a side x side grid of the plane on
    [-extent, extent]^2 -> (cameras, rows [V, 15], points [side^2, 3], (H, W)).  Camera v stands
    at the angle 2 pi (v + 1/2) / V: the cameras all look straight down with the image's long
    side along x, so no camera sits on an axis of the grid, and the ring's mirror symmetries in
    both axes map cameras to cameras."""
    angles = [2 * np.pi * (v + 0.5) / V for v in range(V)]
    cams = [PlaneCamera(radius * np.cos(a), radius * np.sin(a), height, focal, (W - 1) / 2.0,
                        (H - 1) / 2.0) for a in angles]
    g = np.linspace(-extent, extent, side)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    points = np.stack([gx.reshape(-1), gy.reshape(-1), np.zeros(side * side)], 1).astype(D)
    return cams, pack_cameras(cams), points, (H, W)


def analytic_depths(cams, H, W):
    """[V, H, W] f32: the distance of every pixel's point of the plane z = 0 to the centre."""
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    out = []
    for cam in cams:
        gx, gy = cam.ground_point(X, Y)
        out.append(np.sqrt((gx - cam.cx) ** 2 + (gy - cam.cy) ** 2 + cam.height ** 2).astype(F))
    return np.stack(out)


def cosines(min_angle, max_angle):
    """(cos_lo, cos_hi) of a band of angles in degrees: what raynet_amd.view_selection passes."""
    cos_lo = 0.0 if max_angle == 90.0 else float(np.cos(np.deg2rad(D(max_angle))))
    cos_hi = 1.0 if min_angle == 0.0 else float(np.cos(np.deg2rad(D(min_angle))))
    return min(max(cos_lo, 0.0), 1.0), min(max(cos_hi, 0.0), 1.0)
