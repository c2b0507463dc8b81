"""Taubin smoothing of an indexed triangle mesh, restated (DESIGN.md section 23,
include/raynet_hip.h: rn_mesh_smooth): the ring of the corner table, the step of every vertex in
np.float64 with every operation rounded on its own and in the definition's order, float32 positions
between the steps, the ping-pong sequence of lambda and mu steps with the clamp against the input.
`step` runs the rows of all vertices side by side, position by position -- the vertices of a step
do not depend on each other and the order within a row is kept, so it gives the bits of the plain
loop `step_plain`, which is the definition line by line (tests/test_smooth_truth.py holds the two
against each other).  Also: the border of a mesh by a dictionary of edges, the seeded meshes of the
tests with positions, and the measures of the tests.  Nothing here is taken from the kernels.
"""
import numpy as np

import appearance_truth as at
import components_truth as ct
import isosurface_truth as it

F = np.float32
D = np.float64
INF = float("inf")


# ------------------------------------------------------------------------------ the definition
def ring_of(faces, nv, corners):
    """[3 nf, 2] int32: the two other vertices of the face of every table position's corner, in
    the face's order after it; (-1, -1) for a corner outside [0, 3 nf) or a face with an index
    outside [0, nv)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nf = len(faces)
    ring = np.full((3 * nf, 2), -1, np.int32)
    for k, c in enumerate(np.asarray(corners, np.int64).reshape(-1)[:3 * nf].tolist()):
        if not 0 <= c < 3 * nf:
            continue
        f, slot = c // 3, c % 3
        if all(0 <= int(i) < nv for i in faces[f]):
            ring[k] = faces[f][(slot + 1) % 3], faces[f][(slot + 2) % 3]
    return ring


def _clamp(x, start, max_move):
    with np.errstate(invalid="ignore"):
        lo, hi = start - D(max_move), start + D(max_move)
        x = np.where(x < lo, lo, x)
        return np.where(x > hi, hi, x)              # (a NaN passes both tests)


def step_plain(src, start, offsets, ring, fixed, t, max_move):
    """One step with factor t, the definition line by line: a Python loop over the vertices and
    over the row of each."""
    src = np.asarray(src, F).reshape(-1, 3)
    start = np.asarray(start, F).reshape(-1, 3)
    nv, n = len(src), len(ring)
    dst = np.empty_like(src)
    t = D(t)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(nv):
            p = src[v].astype(D)
            s, m = np.zeros(3, D), 0
            first, last = (min(max(int(o), 0), n) for o in offsets[v:v + 2])
            for k in range(first, last):
                a, b = int(ring[k][0]), int(ring[k][1])
                if a < 0:
                    continue
                s = (s + src[a].astype(D)) + src[b].astype(D)
                m = m + 2
            if m == 0 or (fixed is not None and fixed[v]):
                dst[v] = src[v]
            else:
                x = p + t * (s / D(m) - p)
                dst[v] = _clamp(x, start[v].astype(D), max_move).astype(F)
    return dst


def step(src, start, offsets, ring, fixed, t, max_move):
    """One step with factor t: the rows of all vertices side by side, position by position."""
    src = np.asarray(src, F).reshape(-1, 3)
    start = np.asarray(start, F).reshape(-1, 3)
    nv, n = len(src), len(ring)
    offsets = np.asarray(offsets, np.int64)
    first, last = np.clip(offsets[:-1], 0, n), np.clip(offsets[1:], 0, n)
    P = src.astype(D)
    s, m = np.zeros((nv, 3), D), np.zeros(nv, np.int64)
    j = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            live = np.nonzero(first + j < last)[0]
            if not len(live):
                break
            ab = ring[first[live] + j].astype(np.int64)
            ok = ab[:, 0] >= 0
            live, ab = live[ok], ab[ok]
            s[live] = (s[live] + P[ab[:, 0]]) + P[ab[:, 1]]
            m[live] = m[live] + 2
            j += 1
        stay = m == 0
        if fixed is not None:
            stay = stay | (np.asarray(fixed).reshape(-1) != 0)
        x = P + D(t) * (s / np.where(stay, 1, m).astype(D)[:, None] - P)
        moved = _clamp(x, start.astype(D), max_move).astype(F)
    dst = src.copy()
    dst[~stay] = moved[~stay]
    return dst


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed=None, max_move=INF,
           offsets=None, corners=None, one_step=step):
    """-> [nv, 3] float32: rn_mesh_smooth.  fixed: [nv] of 0 / non-zero, or None.  offsets,
    corners: a corner table of the caller's (garbage included); default: the mesh's own."""
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv = len(vertices)
    if offsets is None:
        offsets, corners = at.corner_table(faces, nv)
    ring = ring_of(faces, nv, corners)
    now = vertices.copy()
    for _ in range(int(iterations)):
        now = one_step(now, vertices, offsets, ring, fixed, lam, max_move)
        if mu != 0:
            now = one_step(now, vertices, offsets, ring, fixed, mu, max_move)
    return now


def boundary_vertices(faces, nv):
    """[nv] bool: the vertices on an edge (an undirected pair of two different vertices of a face)
    that lies in exactly one face; a face with an index outside [0, nv) has no edges."""
    count = {}
    for a, b, c in np.asarray(faces, np.int64).reshape(-1, 3).tolist():
        if not all(0 <= i < nv for i in (a, b, c)):
            continue
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                key = (min(p, q), max(p, q))
                count[key] = count.get(key, 0) + 1
    mask = np.zeros(nv, bool)
    for (p, q), n in count.items():
        if n == 1:
            mask[p] = mask[q] = True
    return mask


# ------------------------------------------------------------------------------ the meshes
def positions(nv, seed):
    """[nv, 3] float32 positions, seeded: the vertex index along x plus noise."""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(nv, 3))
    p[:, 0] += np.arange(nv)
    return p.astype(F)


def strip(nv, seed, permuted=False):
    """The strip of components_truth with positions -> (vertices, faces); permuted: vertex ids
    permuted (the positions go along) and the faces shuffled."""
    faces, v = ct.strip(nv), positions(nv, seed)
    if permuted:
        faces, order = ct.shuffled(faces, nv, seed)
        moved = np.empty_like(v)
        moved[order] = v
        v = moved
    return v, faces


def star(nf, seed, hub_last=False):
    faces, nv = ct.star(nf, hub_last)
    return positions(nv, seed), faces


def flat_patch(n=9, z=1.25):
    """An n x n patch of the plane z, two triangles per square, x and y multiples of 0.25 ->
    (vertices, faces)."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([0.25 * i, 0.5 * j, np.full_like(i, z, dtype=D)], -1).reshape(-1, 3).astype(F)
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([q, q + n, q + 1], 1), np.stack([q + 1, q + n, q + n + 1], 1)])
    return v, faces.astype(np.int32)


BALL_GRID, BALL_CENTRE, BALL_RADIUS = (24, 22, 20), (11.3, 10.1, 9.6), 7.2


def binary_ball_field():
    """Belief 0.9 inside the ball, 0.1 outside: what the MRF gives around the threshold."""
    return np.where(it._radius(BALL_GRID, BALL_CENTRE) < BALL_RADIUS, 0.9, 0.1).astype(F)


def binary_ball():
    """The closed iso-surface 0.5 of the binary ball in the unit frame -> (vertices, faces): 2908
    vertices, 5812 faces, terraced."""
    bbox, axes = it.unit_frame(BALL_GRID)
    return it.extract(binary_ball_field(), 0.5, True, axes, bbox)


def with_bad_faces(faces, nv, seed, fraction=0.05):
    return ct.with_garbage(faces, nv, seed, fraction)


def with_bad_corners(corners, nf, seed, fraction=0.05):
    """A copy of `corners` with `fraction` of the entries replaced by one of -1, 3 nf, 2^31 - 1."""
    rng = np.random.default_rng(seed)
    out = np.array(corners, np.int64)
    hit = rng.random(len(out)) < fraction
    out[hit] = rng.choice(np.array([-1, 3 * nf, 2 ** 31 - 1], np.int64), int(hit.sum()))
    return out.astype(np.int32), hit


# ------------------------------------------------------------------------------ the measures
def mean_angle_to_radial(vertices, faces, centre, normals=None):
    """Degrees: the mean angle between the vertex normals (area-weighted, restated) and the
    direction from `centre`, over the vertices with a normal."""
    v = np.asarray(vertices, D).reshape(-1, 3)
    n = (at.area_normals(vertices, faces) if normals is None else np.asarray(normals)).astype(D)
    r = v - np.asarray(centre, D)
    ln, lr = np.sqrt((n * n).sum(1)), np.sqrt((r * r).sum(1))
    ok = (ln > 0) & (lr > 0)
    cos = (n[ok] * r[ok]).sum(1) / (ln[ok] * lr[ok])
    return float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))).mean())


def clamp_bounds(vertices, max_move):
    """(lo, hi) float32: the clamp's fp64 bounds in -+ max_move rounded to float32 -- what every
    coordinate of a result lies between, exactly (rounding is monotone)."""
    v = np.asarray(vertices, F).astype(D)
    with np.errstate(invalid="ignore", over="ignore"):
        return (v - D(max_move)).astype(F), (v + D(max_move)).astype(F)


def mean_radial_error(vertices, centre, radius):
    r = np.sqrt(((np.asarray(vertices, D) - np.asarray(centre, D)) ** 2).sum(1))
    return float(np.abs(r - radius).mean())
