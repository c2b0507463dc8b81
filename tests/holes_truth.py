"""rn_mesh_fill_holes restated twice in NumPy (the definition is in include/raynet_hip.h; DESIGN.md
section 25): `fill_plain`, a Python loop -- a dictionary of the undirected edges, a sequential
union-find, the walk -- and `fill`, vectorised -- sorted edge keys, label propagation, all loops
walked in step.  Both give (new_vertices (k, 3) float32, new_faces (m, 3) int32, source [k] int32,
counts [5] int64) and agree to the bit (tests/test_holes_truth.py); the kernels are held to `fill`.
Below them the meshes the tests share."""
import numpy as np

import appearance_truth as at
import isosurface_truth as it
import smooth_truth as st

F = np.float32
D = np.float64
NO_EDGE = 2 ** 31 - 1
COUNTS = ("filled", "new_faces", "loops", "not_simple", "boundary_edges")


def counting(faces, nv):
    """[nf] bool: the faces with three indices in [0, nv) that differ pairwise."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < nv)).all(1)
    return inside & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


# --------------------------------------------------------------------------- the Python loop
def fill_plain(vertices, faces, max_edges):
    v = np.asarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    nv = len(v)
    finite = np.isfinite(v).all(1)
    counts_in = counting(faces, nv).tolist()
    in_faces = {}
    for face, ok in zip(f, counts_in):
        if ok:
            for s in range(3):
                p, q = face[s], face[(s + 1) % 3]
                key = (min(p, q), max(p, q))
                in_faces[key] = in_faces.get(key, 0) + 1
    half = []                                   # the boundary half-edges (h, a, b), ascending h
    for i, (face, ok) in enumerate(zip(f, counts_in)):
        if ok:
            for s in range(3):
                p, q = face[s], face[(s + 1) % 3]
                if in_faces[(min(p, q), max(p, q))] == 1:
                    half.append((3 * i + s, p, q))
    parent = list(range(nv))

    def root(x):
        while parent[x] != x:
            x = parent[x]
        return x

    out_deg, in_deg, way_out = [0] * nv, [0] * nv, {}
    for h, a, b in half:
        out_deg[a] += 1
        in_deg[b] += 1
        if a not in way_out:                    # (ascending h: the first is the smallest)
            way_out[a] = b
        ra, rb = root(a), root(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    edges, bad = {}, set()
    for h, a, b in half:
        r = root(a)
        edges[r] = edges.get(r, 0) + 1
        for x in (a, b):
            if out_deg[x] != 1 or in_deg[x] != 1 or not finite[x]:
                bad.add(r)
    new_vertices, new_faces, source = [], [], []
    for r in sorted(edges):
        E = edges[r]
        if r in bad or not 3 <= E <= max_edges:
            continue
        k = len(source)
        sums, x = [0.0, 0.0, 0.0], r
        for _ in range(E):
            for axis in range(3):
                sums[axis] = sums[axis] + float(v[x, axis])
            new_faces.append((way_out[x], x, nv + k))
            x = way_out[x]
        assert x == r
        new_vertices.append([F(s / float(E)) for s in sums])
        source.append(r)
    counts = np.array([len(source), len(new_faces), len(edges), len(bad), len(half)], np.int64)
    return (np.array(new_vertices, F).reshape(-1, 3), np.array(new_faces, np.int32).reshape(-1, 3),
            np.array(source, np.int32), counts)


# --------------------------------------------------------------------------- vectorised
def boundary_half_edges(faces, nv):
    """(h, a, b): the boundary half-edges h = 3 f + s, ascending, from a to b."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    valid = np.repeat(counting(f, nv), 3)
    h = np.nonzero(valid)[0]
    keys = np.minimum(a[h], b[h]) * nv + np.maximum(a[h], b[h])
    _, inverse, n = np.unique(keys, return_inverse=True, return_counts=True)
    h = h[n[inverse.reshape(-1)] == 1]
    return h, a[h], b[h]


def loop_labels(a, b, nv):
    """[nv] int64: the smallest vertex every vertex reaches over the edges a[i] -- b[i]."""
    label = np.arange(nv, dtype=np.int64)
    while True:
        low = np.minimum(label[a], label[b])
        new = label.copy()
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def fill(vertices, faces, max_edges):
    v = np.asarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(v)
    head = f[:, [1, 2, 0]].reshape(-1)
    h, a, b = boundary_half_edges(f, nv)
    out_deg, in_deg = np.bincount(a, minlength=nv), np.bincount(b, minlength=nv)
    out_edge = np.full(nv, NO_EDGE, np.int64)
    np.minimum.at(out_edge, a, h)
    label = loop_labels(a, b, nv)
    edges = np.bincount(label[a], minlength=nv)
    plain = (out_deg == 1) & (in_deg == 1) & np.isfinite(v).all(1)
    bad = np.bincount(label[a], weights=~(plain[a] & plain[b]), minlength=nv) > 0
    filled = (edges >= 3) & (edges <= max_edges) & ~bad
    roots = np.nonzero(filled)[0]
    E = edges[roots]
    base = np.cumsum(E) - E
    new_faces = np.zeros((int(E.sum()), 3), np.int64)
    sums = np.zeros((len(roots), 3), D)
    now = roots.copy()
    for j in range(int(E.max()) if len(E) else 0):
        on = j < E
        nxt = head[out_edge[now[on]]]
        sums[on] = sums[on] + v[now[on]].astype(D)
        new_faces[base[on] + j] = np.stack([nxt, now[on], nv + np.nonzero(on)[0]], 1)
        now[on] = nxt
    assert np.array_equal(now, roots)
    centres = (sums / E[:, None].astype(D)).astype(F)
    counts = np.array([len(roots), len(new_faces), int((edges > 0).sum()),
                       int((bad & (edges > 0)).sum()), len(h)], np.int64)
    return centres.reshape(-1, 3), new_faces.astype(np.int32), roots.astype(np.int32), counts


def filled_mesh(vertices, faces, max_edges):
    """-> (vertices, faces, source, stats): the caller's mesh after the call."""
    new_vertices, new_faces, source, counts = fill(vertices, faces, max_edges)
    return (np.concatenate([np.asarray(vertices, F).reshape(-1, 3), new_vertices]),
            np.concatenate([np.asarray(faces, np.int32).reshape(-1, 3), new_faces]), source,
            {name: int(c) for name, c in zip(COUNTS, counts)})


def corner_table(faces, nv):
    """appearance.corner_table for faces that may hold garbage: the corners that name a vertex of
    [0, nv) sorted by it, ascending within a vertex, the others behind them (no row reaches them)."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    inside = (flat >= 0) & (flat < nv)
    if inside.all():
        return at.corner_table(faces, nv)
    key = np.where(inside, flat, nv)
    corners = np.argsort(key, kind="stable").astype(np.int32)
    offsets = np.zeros(nv + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(flat[inside], minlength=nv))
    return offsets.astype(np.int32), corners


def same(got, want):
    """Whether two results (new_vertices, new_faces, source, counts) have the same bits."""
    return (np.array_equal(np.ascontiguousarray(got[0], F).view(np.uint32),
                           np.ascontiguousarray(want[0], F).view(np.uint32)) and
            got[0].shape == want[0].shape and
            all(np.array_equal(np.asarray(g), np.asarray(w)) and np.asarray(g).shape == np.asarray(w).shape
                for g, w in zip(got[1:], want[1:])))


def directed_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed(faces):
    """Every directed half-edge occurs once and has its opposite."""
    de = directed_edges(faces)
    forward = set(map(tuple, de.tolist()))
    return len(forward) == len(de) and all((q, p) in forward for p, q in forward)


# ------------------------------------------------------------------------------ the meshes
def open_tetrahedron():
    """A tetrahedron without its face (1, 2, 3): three faces around vertex 0, wound outwards."""
    v = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-0.5, 0.75, 0.0], [-0.5, -0.75, 0.125]], F)
    return v, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1]], np.int32)


def tube(n, seed=0):
    """An open tube of n segments: two rings of n vertices, 2 n faces, noise on the positions."""
    rng = np.random.default_rng(seed + n)
    angle = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(angle), np.sin(angle), np.zeros(n)], 1)
    v = np.concatenate([ring, ring + [0.0, 0.0, 1.0]]) + 0.01 * rng.normal(size=(2 * n, 3))
    i = np.arange(n)
    j = (i + 1) % n
    faces = np.concatenate([np.stack([i, j, n + j], 1), np.stack([i, n + j, n + i], 1)])
    return v.astype(F), faces.astype(np.int32)


def sheet(w, h, removed=(), seed=0):
    """A height field over w x h cells, two faces per cell, without the cells (x, y) of `removed`;
    vertex y (w + 1) + x lies at (x, y, height): counter-clockwise seen from +z."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w + 1), np.arange(h + 1), indexing="xy")
    z = 0.3 * np.sin(0.7 * x) * np.cos(0.4 * y) + 0.05 * rng.normal(size=x.shape)
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(F)
    keep = np.ones((h, w), bool)
    for cx, cy in removed:
        keep[cy, cx] = False
    cy, cx = np.nonzero(keep)
    q = cy * (w + 1) + cx
    faces = np.stack([np.stack([q, q + 1, q + w + 2], 1), np.stack([q, q + w + 2, q + w + 1], 1)], 1)
    return v, faces.reshape(-1, 3).astype(np.int32)


PUNCHED = ((2, 2), (3, 2), (6, 5), (9, 3), (9, 4))
BOW_TIE = ((2, 2), (3, 3), (6, 1))


def punched_sheet():
    return sheet(12, 9, PUNCHED, seed=1)


def bow_tie_sheet():
    return sheet(8, 8, BOW_TIE, seed=2)


def raster_sheet(n, step, seed=3):
    """An n x n sheet with every cell (x, y), x and y multiples of `step` and at least `step`,
    removed."""
    at_ = range(step, n - 1, step)
    return sheet(n, n, [(x, y) for x in at_ for y in at_], seed=seed)


def face_next_to(faces, a, b):
    """The row of the face that holds the half-edge a -> b."""
    f = np.asarray(faces, np.int64)
    de = np.stack([f, f[:, [1, 2, 0]]], -1)
    return int(np.nonzero(((de[..., 0] == a) & (de[..., 1] == b)).any(1))[0][0])


def flipped_rim():
    """The punched sheet with one face at the hole of cell (6, 5) turned over."""
    v, f = punched_sheet()
    row = face_next_to(f, 71, 84)
    f = f.copy()
    f[row] = f[row][::-1]
    return v, f


def nan_rim():
    """The punched sheet with a NaN coordinate in a vertex of the hole of cell (6, 5)."""
    v, f = punched_sheet()
    v = v.copy()
    v[72, 1] = np.nan
    return v, f


def doubled_face():
    """The punched sheet with a face at the hole of cell (6, 5) twice."""
    v, f = punched_sheet()
    return v, np.concatenate([f, f[[face_next_to(f, 71, 84)]]])


def with_garbage(faces, nv, seed=5):
    """The faces with rows that do not count between them: indices out of range and repeated."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces, np.int32)
    junk = np.array([[0, 1, nv], [-1, 2, 3], [4, 4, 5], [6, 7, 6], [2 ** 31 - 1, 0, 1],
                     [-2 ** 31, 1, 2], [8, 9, 9], [3, 3, 3]], np.int32)
    where = np.sort(rng.integers(0, len(f) + 1, size=len(junk)))
    return np.insert(f, where, junk, axis=0)


def cut_ball():
    """The open iso-surface of isosurface_truth's cut ball: open where the grid ends."""
    field = it.cut_ball()
    bbox, axes = it.unit_frame(field.shape)
    return it.extract(field, 0.5, False, axes, bbox)


def permuted(faces, seed=7):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.asarray(faces, np.int32)[rng.permutation(len(faces))])


def cases():
    """name -> (vertices, faces, max_edges): the meshes the truths and the kernels are compared on."""
    out = {"open_tetrahedron": open_tetrahedron() + (3,)}
    for n in (3, 63, 64, 65, 300):
        out["tube_%d" % n] = tube(n) + (300,)
    out["punched_sheet"] = punched_sheet() + (10,)
    out["punched_sheet_rim_too"] = punched_sheet() + (42,)
    out["punched_sheet_triangles_only"] = punched_sheet() + (3,)
    out["bow_tie"] = bow_tie_sheet() + (10,)
    out["flipped_rim"] = flipped_rim() + (10,)
    out["nan_rim"] = nan_rim() + (10,)
    out["doubled_face"] = doubled_face() + (10,)
    v, f = punched_sheet()
    out["garbage"] = (v, with_garbage(f, len(v)), 10)
    out["cut_ball"] = cut_ball() + (64,)
    return out
