"""rn_mesh_simplify restated in NumPy (include/raynet_hip.h): vertex clustering
on a uniform grid, each cluster at the mean of its members, the mean from fixed-point integer
sums.  `simplify_plain` is the definition line by line in a Python loop, `simplify` the same with
np.add.at / np.minimum.at; both give the bits the kernels have to give.  `unique_faces` is the
dictionary the torch route of raynet_amd.simplify.unique_faces is held to.  The generators are
those of the smoothing's and the components' truths."""
import numpy as np

import components_truth as ct
import isosurface_truth as it
import smooth_truth as st

F = np.float32
D = np.float64
I = np.int32
ONE = D(2097152.0)          # 2^21


def _grid(origin, cell, dims):
    origin = np.broadcast_to(np.asarray(origin, D), (3,)).copy()
    cell = np.broadcast_to(np.asarray(cell, D), (3,)).copy()
    dims = np.asarray(dims, np.int64).reshape(3)
    return origin, cell, dims


def cells_of(vertices, origin, cell, dims):
    """-> (cell [nv] int64, -1 for a singleton; q [nv, 3] int64; w [nv, 3] uint64)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    origin, cell, dims = _grid(origin, cell, dims)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v.astype(D) - origin) / cell
        q = np.floor(t)
        u = t - q
        binned = (np.isfinite(t) & (q >= 0) & (q < dims.astype(D))).all(1)
        qi = np.where(binned[:, None], q, 0.0).astype(np.int64)
        w = np.where(binned[:, None], np.rint(u * ONE), 0.0).astype(np.uint64)
    c = (qi[:, 0] * dims[1] + qi[:, 1]) * dims[2] + qi[:, 2]
    return np.where(binned, c, -1), qi, w


def _mean(origin, cell, q, S, n):
    """x = origin + cell * (q + (S / n) / 2^21), one rounding per operation, as float32."""
    return (origin + cell * (q.astype(D) + (S.astype(D) / n.astype(D)) / ONE)).astype(F)


def _finish(v, faces, key, position_of):
    """The faces, the used clusters and the outputs from every vertex's cluster key (the smallest
    member) and a function giving the position of the cluster of key k."""
    nv = len(v)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < nv)).all(1)
    k = key[np.where(valid[:, None], f, 0)]
    kept = valid & (k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])
    used = np.zeros(nv, bool)
    used[k[kept].reshape(-1)] = True
    source = np.flatnonzero(used)
    index = np.full(nv, -1, np.int64)
    index[source] = np.arange(len(source))
    out = np.empty((len(source), 3), F)
    for o, s in enumerate(source):
        out[o] = position_of(int(s))
    return out, index[k[kept]].astype(I).reshape(-1, 3), source.astype(I), index[key].astype(I)


def simplify_plain(vertices, faces, origin, cell, dims):
    """The definition line by line -> (vertices_out, faces_out, source, cluster)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    origin, cell, dims = _grid(origin, cell, dims)
    nv = len(v)
    table = {}
    cell_of = [-1] * nv
    where = {}
    for i in range(nv):
        q, w, binned = [0, 0, 0], [0, 0, 0], True
        for k in range(3):
            with np.errstate(invalid="ignore", over="ignore"):
                t = (D(v[i, k]) - origin[k]) / cell[k]
                fl = np.floor(t)
            if not (np.isfinite(t) and 0 <= fl < dims[k]):
                binned = False
                continue
            q[k] = int(fl)
            w[k] = int(np.rint((t - fl) * ONE))
        if not binned:
            continue
        c = (q[0] * int(dims[1]) + q[1]) * int(dims[2]) + q[2]
        cell_of[i] = c
        where[c] = q
        entry = table.setdefault(c, [i, 0, [0, 0, 0]])
        entry[0] = min(entry[0], i)
        entry[1] += 1
        for k in range(3):
            entry[2][k] += w[k]
    key = np.array([i if cell_of[i] < 0 else table[cell_of[i]][0] for i in range(nv)], np.int64)

    def position_of(s):
        c = cell_of[s]
        if c < 0 or table[c][1] == 1:
            return v[s]
        _, n, S = table[c]
        return [F(origin[k] + cell[k] * (D(where[c][k]) + (D(S[k]) / D(n)) / ONE))
                for k in range(3)]

    return _finish(v, faces, key.reshape(nv), position_of)


def simplify(vertices, faces, origin, cell, dims):
    """The same, vectorised -> (vertices_out, faces_out, source, cluster)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    origin, cell, dims = _grid(origin, cell, dims)
    nv = len(v)
    c, q, w = cells_of(v, origin, cell, dims)
    binned = np.flatnonzero(c >= 0)
    cells, slot = np.unique(c[binned], return_inverse=True)
    rep = np.full(len(cells), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(rep, slot, binned)
    n = np.zeros(len(cells), np.int64)
    np.add.at(n, slot, 1)
    S = np.zeros((len(cells), 3), np.uint64)
    np.add.at(S, slot, w[binned])
    key = np.arange(nv, dtype=np.int64)
    key[binned] = rep[slot]
    slot_of = np.full(nv, -1, np.int64)
    slot_of[binned] = slot
    means = _mean(origin, cell, q[rep], S, np.maximum(n, 1)[:, None]) if len(cells) else \
        np.zeros((0, 3), F)

    def position_of(s):
        j = slot_of[s]
        return v[s] if j < 0 or n[j] == 1 else means[j]

    return _finish(v, faces, key, position_of)


def unique_faces(faces):
    """The faces with the first of every group kept, a group being the faces that name the same
    three vertices in any order or orientation; the order is kept -> (faces, kept [nf] bool)."""
    f = np.asarray(faces).reshape(-1, 3)
    seen, keep = {}, np.zeros(len(f), bool)
    for i, row in enumerate(f):
        k = tuple(sorted(int(x) for x in row))
        if k not in seen:
            seen[k] = i
            keep[i] = True
    return f[keep], keep


def compact_unreferenced(vertices, faces):
    """The vertices a valid face names, in their order, and the faces renumbered: what a cell so
    small that every vertex is alone in it has to give -> (vertices, faces, source, cluster)."""
    v = np.asarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    kept = ((f >= 0) & (f < len(v))).all(1)
    kept &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    used = np.zeros(len(v), bool)
    used[f[kept].reshape(-1)] = True
    source = np.flatnonzero(used)
    index = np.full(len(v), -1, np.int64)
    index[source] = np.arange(len(source))
    return v[source], index[f[kept]].astype(I).reshape(-1, 3), source.astype(I), index.astype(I)


# ------------------------------------------------------------------------------- the meshes
def grid_around(vertices, cell):
    """(origin, cell [3], dims) of a grid of cells `cell` (a number or three) that covers the finite
    vertices, anchored at multiples of the cell: raynet_amd.simplify.cluster_grid, restated."""
    v = np.asarray(vertices, F).reshape(-1, 3).astype(D)
    cell = np.broadcast_to(np.asarray(cell, D), (3,)).copy()
    origin, dims = np.zeros(3, D), np.ones(3, np.int64)
    for k in range(3):
        x = v[:, k][np.isfinite(v[:, k])]
        if len(x):
            origin[k] = np.floor(x.min() / cell[k]) * cell[k]
            dims[k] = max(int(np.floor((x.max() - origin[k]) / cell[k])) + 1, 1)
    return origin, cell, dims.astype(I)


def cut_ball_mesh():
    """The open iso-surface of isosurface_truth.cut_ball() in the unit frame -> (vertices, faces)."""
    field = it.cut_ball()
    bbox, axes = it.unit_frame(field.shape)
    return it.extract(field, 0.5, False, axes, bbox)


def thin_sheet(n=9):
    """Two flat patches an eighth apart, facing away from each other: with cells of a half both
    sides fall into the same cells and every face of one side doubles one of the other ->
    (vertices, faces)."""
    v, f = st.flat_patch(n, z=1.0)
    back = np.array(v, F)
    back[:, 2] = 1.125
    return np.concatenate([v, back]), np.concatenate([f, f[:, ::-1] + len(v)]).astype(I)


def one_cell_cloud(n, seed):
    """n vertices inside the unit cell at (3, 4, 5) and a strip over them -> (vertices, faces)."""
    rng = np.random.default_rng(seed)
    v = (np.array([3.0, 4.0, 5.0]) + rng.uniform(0.01, 0.99, size=(n, 3))).astype(F)
    return v, ct.strip(n)


def spread_cloud(n, seed):
    """n vertices, one per unit cell along x (noise inside the cell), and a strip over them."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 0.95, size=(n, 3))
    v[:, 0] += np.arange(n)
    return v.astype(F), ct.strip(n)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """All four arrays of two results equal, the vertices by their bits."""
    return (np.array_equal(bits(a[0]), bits(b[0])) and a[0].shape == b[0].shape and
            all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[1:], b[1:])))


def components_count(faces, nv):
    return ct.bfs_count(faces, nv)
