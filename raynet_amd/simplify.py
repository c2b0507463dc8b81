"""Simplification of a surface mesh by vertex clustering (Rossignac and Borrel): the vertices that
share a cell of a uniform grid become one vertex at their mean, the faces that lose a corner that
way vanish, and so do the vertices no face is left for.  Marching
tetrahedra put a vertex on every lattice edge the surface crosses; cells of two voxel sides take
a mesh to a fifth of its faces, and every later stage -- smoothing, normals, colours, the BVH, the
file -- pays per face.

The clustering is HIP (csrc/raynet_simplify.inl; the definition is in include/raynet_hip.h at
rn_mesh_simplify): integer atomics per cell, fixed-point sums, the grid-level scan -- one fixed
result, to the bit.  Here is the plumbing: the grid of a mesh (`cluster_grid`, anchored at world
multiples of the cell so that a translated crop clusters the same way) and the duplicate faces a
collapsed thin sheet leaves behind (`unique_faces`: one sort of canonical keys).

With placement="quadric" a second HIP stage (csrc/raynet_quadric.inl; rn_mesh_place_quadric,
DESIGN.md section 28) moves every cluster vertex from the mean to the minimiser of its summed
squared distances to the planes of the faces around the cluster: the mean of the points around a
crease lies inside the crease, the minimiser on it.  On smooth surfaces it gains nothing in vertex
distance (tangent planes meet outside a sphere), so the mean stays the default.

There is no CPU route: without a GPU `simplify_mesh` raises RaynetHipError.
"""
import numpy as np
import torch

from .appearance import _context, _dev, check_face_indices, faces_tensor

MAX_CELLS = 1 << 28         # 8 GiB of table at the 32 bytes a cell has in the workspace
CELL_BYTES = 32             # S_x, S_y, S_z u64 | rep i32 | n i32
PLACEMENTS = ("mean", "quadric")
REGULARIZATION = 2.0 ** -10         # the pull towards the mean, as a share of the summed weights
MIN_REGULARIZATION = 2.0 ** -20     # what rn_mesh_place_quadric takes: [2^-20, 1]
MAX_MOVE = 1.0                      # cell sides, per axis


def _cell3(cell):
    c = np.asarray(cell, np.float64)
    if c.shape not in ((), (3,)) or not np.all(np.isfinite(c)) or not np.all(c > 0.0):
        raise ValueError("cell: a positive, finite number or three, got %r" % (cell,))
    return np.broadcast_to(c, (3,)).astype(np.float64)


def cluster_grid(vertices, cell, origin=None):
    """-> (origin [3] float64, cell [3] float64, dims [3] int32): the grid of cells with sides
    `cell` (a number, or one per axis) that covers the finite coordinates of `vertices`.  Without
    `origin` the grid starts at floor(min / cell) * cell per axis: the cells are anchored at world
    multiples of the cell, whatever part of a surface the mesh holds.  An axis without a finite
    coordinate gets one cell at 0.  ValueError naming `cell` if the grid would have more than 2^28
    cells (8 GiB of table at 32 bytes per cell)."""
    cell3 = _cell3(cell)
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    if origin is not None:
        origin = np.asarray(origin, np.float64)
        if origin.shape != (3,) or not np.all(np.isfinite(origin)):
            raise ValueError("origin: three finite numbers, got %r" % (origin,))
    start, dims = np.zeros(3, np.float64), np.ones(3, np.float64)
    for k in range(3):
        x = v[:, k][np.isfinite(v[:, k])]
        if origin is not None:
            start[k] = origin[k]
        elif len(x):
            start[k] = np.floor(x.min() / cell3[k]) * cell3[k]
        if len(x):
            dims[k] = max(np.floor((x.max() - start[k]) / cell3[k]) + 1.0, 1.0)
    if not np.all(np.isfinite(start)) or not dims.prod() <= MAX_CELLS:
        raise ValueError("cell: %s gives a grid of %s cells, more than 2^28 (%d bytes of table "
                         "per cell); choose a larger cell" % (tuple(cell3), tuple(dims), CELL_BYTES))
    return start, cell3, dims.astype(np.int32)


def unique_faces(faces):
    """faces (nf, 3) of vertex indices (a tensor on any device, or an array) -> the faces with the
    first of every group kept, on the faces' device; a group is the faces that name the same three
    vertices, in any order or orientation, and the order of the faces is kept.  Clustering a thin
    sheet maps both of its sides to the same triangles: of a collapsed two-sided sheet only one
    side stays -- the first in the faces' order, with its orientation."""
    f = faces_tensor(faces)
    if len(f) == 0:
        return f
    keys = torch.sort(f.to(torch.int64), dim=1).values
    _, group = torch.unique(keys, dim=0, return_inverse=True)       # the one sort
    at = torch.arange(len(f), device=f.device)
    first = torch.full((int(group.max()) + 1,), len(f), dtype=torch.int64, device=f.device)
    first = first.scatter_reduce(0, group, at, reduce="amin")
    return f[first[group] == at]


def mesh_simplify(vertices, faces, origin, cell, dims):
    """The GPU call of `simplify_mesh`: host arrays vertices (nv, 3) float32, faces (nf, 3) int32,
    the grid -> (vertices_out, faces_out, source, cluster) as host arrays."""
    ctx = _context()
    v = _dev(vertices, torch.float32, ctx.device).reshape(-1, 3)
    f = _dev(faces, torch.int32, ctx.device).reshape(-1, 3)
    with torch.cuda.device(ctx.device):
        return tuple(t.cpu().numpy() for t in ctx.mesh_simplify(v, f, origin, cell, dims))


def check_placement(placement, regularization=REGULARIZATION, max_move=MAX_MOVE):
    """ValueError, naming the argument, for a placement that is not one of PLACEMENTS and for what
    rn_mesh_place_quadric would refuse -> (regularization, max_move) as floats."""
    if placement not in PLACEMENTS:
        raise ValueError("placement: one of %s, got %r" % (", ".join(PLACEMENTS), placement))
    try:
        r = float(regularization)
    except (TypeError, ValueError):
        raise ValueError("regularization: a number in [2^-20, 1], got %r" % (regularization,))
    if not MIN_REGULARIZATION <= r <= 1.0:
        raise ValueError("regularization: a number in [2^-20, 1], got %r" % (regularization,))
    try:
        m = float(max_move)
    except (TypeError, ValueError):
        raise ValueError("max_move: a positive number of cell sides or inf, got %r" % (max_move,))
    if not m > 0.0:
        raise ValueError("max_move: a positive number of cell sides or inf, got %r" % (max_move,))
    return r, m


def mesh_place_quadric(vertices, faces, cluster, positions, cell, regularization, max_move):
    """The second GPU call of `simplify_mesh` with placement="quadric": host arrays of the input
    mesh, `cluster` [nv] int32 and the mean positions (nv', 3) float32 that `mesh_simplify`
    returned, the cell's sides [3] -> (positions (nv', 3) float32, counts [2] int64: the vertices
    that moved, the vertices of two or more members whose placement was refused) as host arrays."""
    ctx = _context()
    v = _dev(vertices, torch.float32, ctx.device).reshape(-1, 3)
    f = _dev(faces, torch.int32, ctx.device).reshape(-1, 3)
    c = _dev(cluster, torch.int32, ctx.device).reshape(-1)
    p = _dev(positions, torch.float32, ctx.device).reshape(-1, 3)
    with torch.cuda.device(ctx.device):
        out, counts = ctx.mesh_place_quadric(v, f, c, p, cell, regularization, max_move)
        return out.cpu().numpy(), counts


def placement_stats(before, after, cell, counts):
    """What `simplify_mesh` reports of a quadric placement: the counts of the entry and the
    farthest a coordinate moved from the mean, in sides of the cell along its axis."""
    moved = np.abs(np.asarray(after, np.float64) - np.asarray(before, np.float64)) / cell
    moved = moved[np.isfinite(moved)]
    return {"moved": int(counts[0]), "fell_back": int(counts[1]),
            "farthest_move": float(moved.max()) if moved.size else 0.0}


def simplify_mesh(vertices, faces, cell, origin=None, drop_duplicate_faces=True,
                  placement="mean", regularization=REGULARIZATION, max_move=MAX_MOVE,
                  return_stats=False):
    """-> (vertices (nv', 3) float32, faces (nf', 3) int32, source [nv'] int32): the mesh
    (vertices (nv, 3), faces (nf, 3)) with the vertices of every cell of `cluster_grid(vertices,
    cell, origin)` merged at their mean; a vertex alone in its cell keeps its bits, a non-finite
    one is a cluster of its own.  Faces with two corners in one cluster vanish, the others keep
    their order and winding; vertices no face is left for vanish, the others keep the order of
    `source`, the smallest input vertex of each.  drop_duplicate_faces: `unique_faces` over the
    result; the vertices that only dropped duplicates used are NOT dropped again (a face and its
    duplicates name the same vertices, so there are none).  ValueError, naming the argument, for
    what rn_mesh_simplify would refuse and for a face index outside the vertices.

    placement: "mean" (the default: exactly the above, one GPU call) or "quadric": every output
    vertex then moves to the point nearest, in the least-squares sense, to the planes of the input
    faces that touch its cluster (`mesh_place_quadric`; the faces the clustering drops count too).
    regularization in [2^-20, 1] pulls it back to the mean, as a share of the faces' summed
    weights -- it is what keeps a vertex on a flat region or along a crease where the planes leave
    it free; max_move > 0 (inf: no limit) bounds the move per axis in cell sides.  Faces, `source`
    and the order of everything are those of "mean".  return_stats: a fourth value, the dict
    {moved, fell_back, farthest_move} of `placement_stats` (zeros for "mean")."""
    regularization, max_move = check_placement(placement, regularization, max_move)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    nv = len(v)
    if nv > 2 ** 31 - 2:
        raise ValueError("vertices: at most 2^31 - 2, got %d" % nv)
    if 3 * len(f) > 2 ** 31 - 1:
        raise ValueError("faces: at most (2^31 - 1) / 3, got %d" % len(f))
    check_face_indices(f, nv)
    start, cell3, dims = cluster_grid(v, cell, origin)
    out_v, out_f, source, cluster = mesh_simplify(v, f, start, cell3, dims)
    stats = {"moved": 0, "fell_back": 0, "farthest_move": 0.0}
    if placement == "quadric" and len(out_v):
        mean = np.ascontiguousarray(out_v, np.float32).reshape(-1, 3)
        out_v, counts = mesh_place_quadric(v, f, cluster, mean, cell3, regularization, max_move)
        stats = placement_stats(mean, out_v, cell3, counts)
    if drop_duplicate_faces and len(out_f):
        device = "cuda" if torch.cuda.is_available() else "cpu"
        out_f = unique_faces(torch.from_numpy(np.ascontiguousarray(out_f)).to(device)).cpu().numpy()
    out = (np.ascontiguousarray(out_v, np.float32).reshape(-1, 3),
           np.ascontiguousarray(out_f, np.int32).reshape(-1, 3),
           np.ascontiguousarray(source, np.int32).reshape(-1))
    return out + (stats,) if return_stats else out
