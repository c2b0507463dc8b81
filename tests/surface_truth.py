"""The truth of the surface queries (raynet_amd/mesh.py: closest_points, sample_surface):
float64 NumPy, brute force over all triangles.  Two independent restatements of the distance
of a point to a triangle -- Ericson's region classification and the minimum of the three
clamped segment distances and the plane projection -- and the restatement of the sampler's
documented hash and formulas.  All functions broadcast: q, a, b, c are
[..., 3] float64."""
import numpy as np


def _dot(x, y):
    return (x * y).sum(-1)


def _sdiv(num, den):
    """num / den where den > 0, else 0."""
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


def closest_ericson(q, a, b, c):
    """(distance, closest point) by the region classification of Ericson, Real-Time Collision
    Detection 5.1.5: vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face, in that
    order.  An edge's region counts only where the edge has a length (its denominator, the
    squared length, is > 0): with a == b every cross term of ab is zero and the unguarded rule
    would claim every point for "edge ab"; a collapsed edge is left to the regions of the
    vertices and of the other edges."""
    q, a, b, c = [np.asarray(x, np.float64) for x in (q, a, b, c)]
    ab, ac = b - a, c - a
    ap, bp, cp = q - a, q - b, q - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    den = va + vb + vc
    v = np.clip(_sdiv(vb, den), 0.0, 1.0)
    w = np.clip(_sdiv(vc, den), 0.0, 1.0 - v)
    # lowest priority first: a later rule overrides an earlier one
    rules = [
        (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0) & ((d4 - d3) + (d5 - d6) > 0),   # edge bc
        (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (d2 - d6 > 0),     # edge ac
        (d6 >= 0) & (d5 <= d6),                                 # vertex c
        (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (d1 - d3 > 0),     # edge ab
        (d3 >= 0) & (d4 <= d3),                                 # vertex b
        (d1 <= 0) & (d2 <= 0),                                  # vertex a
    ]
    w_bc = _sdiv(d4 - d3, (d4 - d3) + (d5 - d6))
    values = [(1.0 - w_bc, w_bc), (0.0, _sdiv(d2, d2 - d6)), (0.0, 1.0),
              (_sdiv(d1, d1 - d3), 0.0), (1.0, 0.0), (0.0, 0.0)]
    for rule, (rv, rw) in zip(rules, values):
        v = np.where(rule, rv, v)
        w = np.where(rule, rw, w)
    p = a + v[..., None] * ab + w[..., None] * ac
    e = q - p
    return np.sqrt(_dot(e, e)), p


def dist_ericson(q, a, b, c):
    return closest_ericson(q, a, b, c)[0]


def _dist_segment(q, p, r):
    d = r - p
    t = np.clip(_sdiv(_dot(q - p, d), _dot(d, d)), 0.0, 1.0)
    e = q - (p + t[..., None] * d)
    return np.sqrt(_dot(e, e))


def dist_segments_plane(q, a, b, c):
    """The minimum of the distances to the three edges (as clamped segments) and, where the
    point's projection onto the plane lies inside the triangle and the normal is non-zero, of
    the distance to the plane."""
    q, a, b, c = [np.asarray(x, np.float64) for x in (q, a, b, c)]
    q, a, b, c = np.broadcast_arrays(q, a, b, c)
    d = np.minimum(np.minimum(_dist_segment(q, a, b), _dist_segment(q, b, c)),
                   _dist_segment(q, c, a))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    inside = (_dot(np.cross(b - a, q - a), n) >= 0) & (_dot(np.cross(c - b, q - b), n) >= 0) & \
             (_dot(np.cross(a - c, q - c), n) >= 0) & (nn > 0)
    plane = np.abs(_dot(q - a, n)) / np.sqrt(np.where(nn > 0, nn, 1.0))
    return np.where(inside, np.minimum(d, plane), d)


def brute_force(Q, A, B, C, fn=dist_ericson, chunk=128):
    """min over all triangles: (distance [n], triangle [n]) for queries Q [n, 3] and triangles
    with vertices A, B, C [T, 3]."""
    Q = np.asarray(Q, np.float64)
    dist = np.empty(len(Q))
    idx = np.empty(len(Q), np.int64)
    for s in range(0, len(Q), chunk):
        d = fn(Q[s:s + chunk, None, :], A[None], B[None], C[None])
        idx[s:s + chunk] = d.argmin(1)
        dist[s:s + chunk] = d.min(1)
    return dist, idx


def brute_force_culled(Q, A, B, C, fn=dist_ericson, chunk=256):
    """brute_force's result, faster: per query, the exact distance is taken only to the
    triangles whose box is not further away than the nearest first vertex -- a triangle
    beyond that cannot hold the minimum (the box distance is a lower bound of the triangle's,
    the distance to a vertex an upper bound of the minimum; 1e-9 relative slack for rounding)."""
    Q = np.asarray(Q, np.float64)
    lo = np.minimum(np.minimum(A, B), C)
    hi = np.maximum(np.maximum(A, B), C)
    dist = np.empty(len(Q))
    idx = np.empty(len(Q), np.int64)
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk, None, :]
        gap = np.maximum(np.maximum(lo[None] - q, q - hi[None]), 0.0)
        lower = np.sqrt((gap * gap).sum(-1))
        upper = np.sqrt(((q - A[None]) ** 2).sum(-1)).min(1)
        qi, ti = np.nonzero(lower <= upper[:, None] * (1 + 1e-9))
        d = fn(Q[s + qi], A[ti], B[ti], C[ti])
        order = np.lexsort((d, qi))
        rows, first = np.unique(qi[order], return_index=True)
        assert len(rows) == q.shape[0]
        dist[s:s + chunk] = d[order][first]
        idx[s:s + chunk] = ti[order][first]
    return dist, idx


def leaf_vertices(leaves):
    """The surface's triangles from a MeshRaycaster's leaves [T, 12] f32 (host array), in the
    ORIGINAL triangle order: a = p0, b = p0 + e1, c = p0 + e2 in float64."""
    L = np.asarray(leaves, np.float32)
    order = np.argsort(L[:, 3].copy().view(np.int32), kind="stable")
    L = L[order].astype(np.float64)
    a = L[:, 0:3]
    return a, a + L[:, 4:7], a + L[:, 8:11]


def file_vertices(tri):
    """The vertices of a triangle array [T, 9] f32 in float64."""
    t = np.asarray(tri, np.float32).astype(np.float64)
    return t[:, 0:3], t[:, 3:6], t[:, 6:9]


def areas(tri):
    """0.5 |e1 x e2| in float64 from the fp32 vertices, the kernel's operation order."""
    a, b, c = file_vertices(tri)
    e1, e2 = b - a, c - a
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


# ---- the sampler's hash and formulas, restated ------------------------------------------------
_G = np.uint64(0x9E3779B97F4A7C15)


def mix64(z):
    """splitmix64's output function on uint64 arrays (arithmetic modulo 2^64)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def uniforms(seed, n):
    """r[k, j] in [0, 1), j = 0, 1, 2: the top 53 bits of
    mix64(mix64(seed + G) + G * (3 k + j + 1))."""
    with np.errstate(over="ignore"):
        key = mix64(np.array([seed], np.int64).view(np.uint64) + _G)
        c = np.uint64(3) * np.arange(n, dtype=np.uint64)[:, None] + \
            np.arange(1, 4, dtype=np.uint64)[None]
        h = mix64(key + _G * c)
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def sample_surface(tri, area_cdf, n, seed):
    """(points [n, 3] f32, triangle [n]) as k_mesh_sample forms them, from the DEVICE's own
    running sum `area_cdf`."""
    r = uniforms(seed, n)
    total = area_cdf[-1]
    x = (np.arange(n, dtype=np.float64) + r[:, 0]) / np.float64(n) * total
    x = np.where(x < total, x, np.nextafter(total, 0.0))
    t = np.searchsorted(area_cdf, x, side="right")          # the first t with cdf[t] > x
    fold = r[:, 1] + r[:, 2] > 1.0
    u = np.where(fold, 1.0 - r[:, 1], r[:, 1])[:, None]
    v = np.where(fold, 1.0 - r[:, 2], r[:, 2])[:, None]
    a, b, c = file_vertices(tri)
    a, b, c = a[t], b[t], c[t]
    return ((a + u * (b - a)) + v * (c - a)).astype(np.float32), t
