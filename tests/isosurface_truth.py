"""The iso-surface of a belief grid by marching tetrahedra, restated in NumPy (DESIGN.md section
19, include/raynet_hip.h: rn_isosurface_count / rn_isosurface_emit): the definition the GPU tests
hold the kernels to bit for bit, and the checks a closed oriented surface has to pass.

Nothing here is taken from the kernels: the orientation of every triangle is derived below, in
float64, from the geometry of the unit tetrahedra (the sign of normal . (outside centroid -
inside centroid)); the positions are np.float32 arithmetic, every operation rounded on its own.
"""
import itertools

import numpy as np

F = np.float32

# the Kuhn split of a cell: corner masks (bit 0: +x, bit 1: +y, bit 2: +z), one tetrahedron per
# permutation of the axes, in lexicographic order
TETS = []
for perm in itertools.permutations(range(3)):
    m, t = 0, [0]
    for axis in perm:
        m |= 1 << axis
        t.append(m)
    TETS.append(t)
assert TETS == [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]


def _xyz(mask):
    return np.array([mask & 1, (mask >> 1) & 1, (mask >> 2) & 1], np.float64)


def _case_triangles(tet, case):
    """Triangles of tetrahedron `tet` (4 corner masks) whose local corner l is inside iff bit l
    of `case`: a list of triangles, each three edges (lower mask, higher mask XOR lower mask)."""
    ins = [l for l in range(4) if (case >> l) & 1]
    out = [l for l in range(4) if not (case >> l) & 1]
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in out]]
    elif len(ins) == 3:
        tris = [[(i, out[0]) for i in ins]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        return []
    towards = np.mean([_xyz(tet[l]) for l in out], 0) - np.mean([_xyz(tet[l]) for l in ins], 0)
    result = []
    for tri in tris:
        mid = [(_xyz(tet[u]) + _xyz(tet[v])) / 2 for u, v in tri]
        normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        s = float(normal @ towards)
        assert abs(s) > 1e-9
        if s < 0:
            tri = [tri[0], tri[2], tri[1]]
        edges = []
        for u, v in tri:
            lo, hi = min(tet[u], tet[v]), max(tet[u], tet[v])
            assert hi & lo == lo and hi != lo
            edges.append((lo, hi ^ lo))
        result.append(edges)
    return result


TABLE = [[_case_triangles(tet, case) for case in range(16)] for tet in TETS]


def padded_axis(axis, lo, hi, g, closed):
    """The coordinates of the lattice points of one axis: the g table entries and, closed, one
    point in front and one behind at the voxel size h = fl(fl(hi - lo) / g)."""
    axis = np.asarray(axis, F)
    assert axis.shape == (g,)
    if not closed:
        return axis
    h = F(F(F(hi) - F(lo)) / F(g))
    return np.concatenate([[F(axis[0] - h)], axis, [F(axis[-1] + h)]]).astype(F)


def extract(belief, iso, closed, axes, bbox):
    """belief [gx][gy][gz] f32, axes: the three tables of voxel centres, bbox [6] ->
    (vertices [nv, 3] f32, faces [nf, 3] int32) in the definition's order."""
    belief = np.asarray(belief, F)
    bbox = np.asarray(bbox, F).reshape(6)
    iso = F(iso)
    c = 1 if closed else 0
    g = belief.shape
    n = tuple(s + 2 * c for s in g)
    empty = np.zeros((0, 3), F), np.zeros((0, 3), np.int32)
    if min(n) < 2:
        return empty                        # no cells: the mesh is empty, vertices included
    val = np.zeros(n, F)
    val[c:c + g[0], c:c + g[1], c:c + g[2]] = belief
    with np.errstate(invalid="ignore"):
        ins = val >= iso                    # NaN: outside
    A = [padded_axis(axes[a], bbox[a], bbox[3 + a], g[a], c) for a in range(3)]
    L = n[0] * n[1] * n[2]
    # edges (p, d) that carry a vertex
    cross = np.zeros((7,) + n, bool)
    for d in range(1, 8):
        o = (d & 1, (d >> 1) & 1, (d >> 2) & 1)
        p = tuple(slice(0, n[a] - o[a]) for a in range(3))
        q = tuple(slice(o[a], n[a]) for a in range(3))
        cross[(d - 1,) + p] = ins[p] != ins[q]
    cr = np.ascontiguousarray(cross.reshape(7, L).T)            # [p][d - 1]
    vid = (np.cumsum(cr.ravel()) - 1).reshape(L, 7)
    pidx, dm1 = np.nonzero(cr)                                  # by p, then by d
    d = dm1 + 1
    ijk = np.unravel_index(pidx, n)
    off = [(d >> a) & 1 for a in range(3)]
    a_ = val[ijk]
    b_ = val[tuple(ijk[a] + off[a] for a in range(3))]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = ((iso - a_).astype(F) / (b_ - a_).astype(F)).astype(F)
        vertices = np.empty((len(pidx), 3), F)
        for a in range(3):
            ap = A[a][ijk[a]]
            aq = A[a][ijk[a] + off[a]]
            moved = (ap + (t * (aq - ap).astype(F)).astype(F)).astype(F)
            vertices[:, a] = np.where(off[a] == 1, moved, ap)
    # triangles of the cells
    m = tuple(s - 1 for s in n)
    lin = np.arange(L).reshape(n)

    def at(mask, arr):
        o = (mask & 1, (mask >> 1) & 1, (mask >> 2) & 1)
        return arr[o[0]:o[0] + m[0], o[1]:o[1] + m[1], o[2]:o[2] + m[2]].reshape(-1)

    inside = [at(mask, ins) for mask in range(8)]
    point = [at(mask, lin) for mask in range(8)]
    rows, keys = [], []
    for ti, tet in enumerate(TETS):
        case = sum(inside[tet[l]].astype(np.int64) << l for l in range(4))
        for cv in range(1, 15):
            cells = np.nonzero(case == cv)[0]
            if not len(cells):
                continue
            for r, tri in enumerate(TABLE[ti][cv]):
                rows.append(np.stack([vid[point[lo][cells], dd - 1] for lo, dd in tri], 1))
                keys.append(cells * 12 + ti * 2 + r)
    if not rows:
        assert len(vertices) == 0
        return empty
    rows, keys = np.concatenate(rows), np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys)
    faces = rows[order]
    # (an index taken from an edge that carries no vertex would be the bug of this file)
    assert faces.min() >= 0 and faces.max() < len(vertices)
    return vertices, np.ascontiguousarray(faces.astype(np.int32))


# ------------------------------------------------------------------- the checks on a surface
def edge_census(faces):
    """(number of undirected edges, how many of them lie in exactly two faces, how many directed
    edges are used more than once, the undirected edges that lie in one face only [k, 2])."""
    f = np.asarray(faces, np.int64)
    if not len(f):
        return 0, 0, 0, np.zeros((0, 2), np.int64)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    _, dcount = np.unique(de, axis=0, return_counts=True)
    ue, ucount = np.unique(np.sort(de, axis=1), axis=0, return_counts=True)
    return len(ue), int((ucount == 2).sum()), int((dcount > 1).sum()), ue[ucount == 1]


def is_closed_and_oriented(vertices, faces):
    """Every undirected edge in exactly two faces, every directed edge exactly once, every
    vertex used."""
    E, two, repeated, _ = edge_census(faces)
    used = np.unique(np.asarray(faces).ravel())
    return E == two and repeated == 0 and len(used) == len(vertices)


def euler_characteristic(vertices, faces):
    return len(vertices) - edge_census(faces)[0] + len(faces)


def signed_volume(vertices, faces):
    """float64: positive where the normals point outwards."""
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ----------------------------------------------------------------------------- the inputs
def unit_frame(grid):
    """bbox and axis tables in which voxel (i, j, k) has its centre at (i, j, k)."""
    bbox = np.array([-0.5, -0.5, -0.5] + [s - 0.5 for s in grid], F)
    return bbox, [np.arange(s, dtype=F) for s in grid]


def _radius(grid, centre):
    i, j, k = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in grid], indexing="ij")
    return np.sqrt((i - centre[0]) ** 2 + (j - centre[1]) ** 2 + (k - centre[2]) ** 2)


def logistic_ball(grid=(12, 11, 10), centre=(5.3, 5.1, 4.6), radius=3.7):
    return (1.0 / (1.0 + np.exp(2.0 * (_radius(grid, centre) - radius)))).astype(F)


def cut_ball():
    return logistic_ball(centre=(1.0, 5.1, 4.6))


def torus(grid=(16, 16, 8), major=5.0, minor=1.8):
    i, j, k = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in grid], indexing="ij")
    cx, cy, cz = [(s - 1) / 2.0 + 0.13 for s in grid]
    ring = np.sqrt((i - cx) ** 2 + (j - cy) ** 2) - major
    dist = np.sqrt(ring ** 2 + (k - cz) ** 2)
    return (1.0 / (1.0 + np.exp(2.0 * (dist - minor)))).astype(F)


def noise(grid=(6, 5, 7), seed=3):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0.1, 0.3, 0.5, 0.7, 0.9], F), size=grid).astype(F)


def planted_voxel(grid=(4, 5, 3), where=(1, 2, 1)):
    b = np.zeros(grid, F)
    b[where] = F(0.9)
    return b


def two_balls(grid=(40, 40, 40)):
    a = logistic_ball(grid, (12.3, 14.1, 20.6), 7.7).astype(np.float64)
    b = logistic_ball(grid, (27.2, 25.4, 17.9), 9.1).astype(np.float64)
    return np.maximum(a, b).astype(F)
