"""The connected components of an indexed triangle mesh, restated sequentially (DESIGN.md section
22, include/raynet_hip.h: rn_mesh_components): a union-find in plain Python over NumPy arrays that
unites by the smaller index and compresses paths, the labels and counts of the definition --
out-of-range faces skipped whole -- the selection of components and the compaction of a mesh, and
the seeded mesh generators of the tests.  Nothing here is taken from the kernels.
"""
import numpy as np

I = np.int32


def counted(faces, nv):
    """[nf] bool: the faces all three indices of which name a vertex."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((faces >= 0) & (faces < nv)).all(1)


def labels_of(faces, nv):
    """[nv] int32: the smallest vertex index of every vertex's component."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(nv))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    def unite(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for a, b, c in faces[counted(faces, nv)].tolist():
        unite(a, b)
        unite(b, c)
    return np.array([find(v) for v in range(nv)], I).reshape(nv)


def components(faces, nv):
    """-> (labels, vertex_counts, face_counts), each [nv] int32, by the definition."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    labels = labels_of(faces, nv)
    vertex_counts = np.bincount(labels, minlength=nv).astype(I)[:nv]
    first = faces[counted(faces, nv), 0]
    face_counts = np.bincount(labels[first], minlength=nv).astype(I)[:nv]
    return labels, vertex_counts, face_counts


def bfs_count(faces, nv):
    """The number of components by a breadth-first search over adjacency lists."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    near = [[] for _ in range(nv)]
    for a, b, c in faces[counted(faces, nv)].tolist():
        near[a] += [b, c]
        near[b] += [a, c]
        near[c] += [a, b]
    seen, n = [False] * nv, 0
    for s in range(nv):
        if seen[s]:
            continue
        n += 1
        seen[s] = True
        queue = [s]
        while queue:
            nxt = []
            for u in queue:
                for w in near[u]:
                    if not seen[w]:
                        seen[w] = True
                        nxt.append(w)
            queue = nxt
    return n


# ------------------------------------------------------------------- selection and compaction
def dense(labels, vertex_counts, face_counts):
    """-> (roots [K] ascending, component [nv] dense id, n_vertices [K], n_faces [K])."""
    labels = np.asarray(labels, np.int64)
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    component = np.searchsorted(roots, labels)
    return roots.astype(I), component.astype(I), np.asarray(vertex_counts, np.int64)[roots], \
        np.asarray(face_counts, np.int64)[roots]


def largest(n_faces, k):
    """The ids of the k components with the most faces, ties to the lower id."""
    n_faces = np.asarray(n_faces, np.int64)
    order = sorted(range(len(n_faces)), key=lambda i: (-int(n_faces[i]), i))
    return np.array(order[:max(int(k), 0)], np.int64)


def select(n_faces, min_faces=None, min_fraction=None, keep_largest=None):
    """[K] bool: the conjunction of the criteria given; no component without faces."""
    n_faces = np.asarray(n_faces, np.int64)
    keep = n_faces > 0
    if min_faces is not None:
        keep &= n_faces >= int(min_faces)
    if min_fraction is not None and len(n_faces):
        keep &= n_faces.astype(np.float64) >= np.float64(min_fraction) * np.float64(n_faces.max())
    if keep_largest is not None:
        top = np.zeros(len(n_faces), bool)
        top[largest(n_faces, keep_largest)] = True
        keep &= top
    return keep


def compact(vertices, faces, keep_faces):
    """The faces of the mask and the vertices they name, renumbered, both in their order ->
    (vertices, faces, used [nv] bool)."""
    vertices = np.asarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, I).reshape(-1, 3)[np.asarray(keep_faces, bool)]
    used = np.zeros(len(vertices), bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return np.ascontiguousarray(vertices[used]), \
        np.ascontiguousarray(new[faces].astype(I)).reshape(-1, 3), used


def filtered(vertices, faces, **criteria):
    """What SurfaceMesh.without_small_components(**criteria) has to give -> (vertices, faces,
    used, K found, k kept)."""
    faces = np.asarray(faces, I).reshape(-1, 3)
    nv = len(np.asarray(vertices).reshape(-1, 3))
    roots, component, _, n_faces = dense(*components(faces, nv))
    keep = select(n_faces, **criteria)
    keep_faces = keep[component[faces[:, 0]]] if len(faces) else np.zeros(0, bool)
    return compact(vertices, faces, keep_faces) + (len(roots), int(keep.sum()))


# ------------------------------------------------------------------------------ the meshes
def strip(nv):
    """The faces (i, i + 1, i + 2): one component, the deepest chase there is."""
    i = np.arange(max(nv - 2, 0), dtype=np.int64)
    return np.stack([i, i + 1, i + 2], 1).astype(I).reshape(-1, 3)


def star(nf, hub_last=False):
    """nf faces that share one vertex (0, or the last one), every other vertex in one face ->
    (faces, nv)."""
    nv = 2 * nf + 1
    i = np.arange(nf, dtype=np.int64)
    if hub_last:
        return np.stack([np.full(nf, nv - 1), 2 * i, 2 * i + 1], 1).astype(I), nv
    return np.stack([np.zeros(nf, np.int64), 2 * i + 1, 2 * i + 2], 1).astype(I), nv


def triangles(n):
    """n disjoint triangles -> (faces, nv)."""
    return np.arange(3 * n, dtype=I).reshape(n, 3), 3 * n


def tetrahedra(n):
    """n disjoint tetrahedra (4 vertices, 4 faces each) -> (faces, nv)."""
    local = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], np.int64)
    return (4 * np.arange(n, dtype=np.int64)[:, None, None] + local).reshape(-1, 3).astype(I), 4 * n


def two_blobs(nf_each, seed):
    """Two random connected blobs of nf_each faces each, joined only by the last face ->
    (faces, nv)."""
    rng = np.random.default_rng(seed)
    nvb = nf_each // 2 + 3

    def blob(offset):
        # face k names vertex k' = 2 + k % (nvb - 2) and two vertices below it: connected
        top = 2 + np.arange(nf_each, dtype=np.int64) % (nvb - 2)
        a = rng.integers(0, top)
        b = rng.integers(0, top)
        a[top == 2], b[top == 2] = 0, 1
        return np.stack([top, a, b], 1) + offset

    bridge = np.array([[nvb - 1, nvb, 2 * nvb - 1]], np.int64)
    return np.concatenate([blob(0), blob(nvb), bridge]).astype(I), 2 * nvb


def renumber(faces, nv, order):
    """The faces with vertex v renamed order[v]; indices outside [0, nv) stay what they are."""
    faces = np.asarray(faces, np.int64)
    order = np.asarray(order, np.int64)
    inside = (faces >= 0) & (faces < nv)
    return np.where(inside, order[np.where(inside, faces, 0)], faces).astype(I)


def reversed_ids(faces, nv):
    return renumber(faces, nv, np.arange(nv)[::-1])


def shuffled(faces, nv, seed):
    """Vertex ids permuted and faces shuffled -> (faces, the permutation new = order[old])."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(nv)
    out = renumber(faces, nv, order)
    return np.ascontiguousarray(out[rng.permutation(len(out))]), order


def with_garbage(faces, nv, seed, fraction=0.05):
    """A copy with one index of `fraction` of the faces replaced by one of -1, nv, 2^31 - 1,
    -2^31 -> (faces, the mask of the planted faces)."""
    rng = np.random.default_rng(seed)
    out = np.array(faces, np.int64).reshape(-1, 3)
    hit = rng.random(len(out)) < fraction
    rows = np.flatnonzero(hit)
    out[rows, rng.integers(0, 3, len(rows))] = rng.choice(
        np.array([-1, nv, 2 ** 31 - 1, -2 ** 31], np.int64), len(rows))
    return out.astype(I), hit


def balls_field(grid=(24, 22, 20)):
    """A float32 field on `grid` with three separated balls of different radii and one
    single-voxel speck, values in [0, 1], 0.5 the surface -> the field."""
    gx, gy, gz = grid
    x, y, z = np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij")
    field = np.zeros(grid, np.float64)
    for (cx, cy, cz), r in [((6.3, 6.1, 6.2), 4.4), ((16.2, 14.9, 12.1), 3.3),
                            ((17.1, 5.2, 5.3), 2.2)]:
        d = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
        field = np.maximum(field, np.clip(0.5 + (r - d) / 2.0, 0.0, 1.0))
    field[4, 17, 15] = 0.9
    return field.astype(np.float32)
