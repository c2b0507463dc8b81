"""The small holes of a surface mesh closed: every simple boundary loop of at most `max_edges`
edges gets a vertex at the mean of its vertices and a fan of faces from that vertex to its edges
(DESIGN.md section 25).  A fused mesh is open where observation ends; an occluded patch, a pixel
below the weight threshold, a NaN voxel inside an otherwise seen surface each leave a small loop of
boundary edges, which costs completeness, pins the smoothing at its ragged rim and shows the back
faces through it.  The long loops -- the outer rim of the surface -- stay open: a loop is told from
a rim by its length alone.

The work is HIP (csrc/raynet_holes.inl; the definition is in include/raynet_hip.h at
rn_mesh_fill_holes): the boundary test by a gather over the corner table that the normals and the
smoothing use, the loops by the union-find of the components, one scan, one walk per filled loop;
integer atomics only -- one fixed result, to the bit.  Here is the plumbing.

There is no CPU route: without a GPU `fill_holes` raises RaynetHipError.
"""
import numpy as np
import torch

from .appearance import _context, _dev, check_face_indices, corner_table

MIN_EDGES, MAX_EDGES = 3, 65536
COUNTS = ("filled", "new_faces", "loops", "not_simple", "boundary_edges")


def check_max_edges(max_edges):
    """ValueError, naming the argument, for what rn_mesh_fill_holes would refuse."""
    if isinstance(max_edges, bool) or int(max_edges) != max_edges or \
            not MIN_EDGES <= int(max_edges) <= MAX_EDGES:
        raise ValueError("max_edges: a whole number in %d..%d, got %r"
                         % (MIN_EDGES, MAX_EDGES, max_edges))
    return int(max_edges)


def mesh_fill_holes(vertices, faces, max_edges):
    """The GPU call of `fill_holes`: host arrays vertices (nv, 3) float32, faces (nf, 3) int32 with
    every index in [0, nv) -> (new_vertices, new_faces, source, counts) as host arrays."""
    ctx = _context("fills holes")
    v = _dev(vertices, torch.float32, ctx.device).reshape(-1, 3)
    f = _dev(faces, torch.int32, ctx.device).reshape(-1, 3)
    with torch.cuda.device(ctx.device):
        offsets, corners = corner_table(f, len(v))
        out = ctx.mesh_fill_holes(v, f, offsets, corners, int(max_edges))
        return tuple(t.cpu().numpy() for t in out[:3]) + (np.asarray(out[3], np.int64),)


def fill_holes(vertices, faces, max_edges):
    """-> (vertices (nv + k, 3) float32, faces (nf + m, 3) int32, source [k] int32, stats): the
    mesh (vertices (nv, 3), faces (nf, 3)) with every simple boundary loop of 3..max_edges edges
    capped.  The input's vertices and faces come first, with their bits and in their order; vertex
    nv + i is the centre of the loop whose smallest vertex is source[i] (ascending), and the new
    faces follow loop by loop, wound like the mesh.  A loop that is not simple -- two holes that
    meet at a vertex, a rim with a flipped face, a loop through a non-finite vertex -- stays open.
    stats: a dict of the five counts `filled`, `new_faces`, `loops`, `not_simple`,
    `boundary_edges`.  ValueError, naming the argument, for what rn_mesh_fill_holes would refuse
    and for a face index outside the vertices."""
    max_edges = check_max_edges(max_edges)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    nv, nf = len(v), len(f)
    if nv > 2 ** 31 - 2:
        raise ValueError("vertices: at most 2^31 - 2, got %d" % nv)
    if 3 * nf > 2 ** 31 - 1:
        raise ValueError("faces: at most (2^31 - 1) / 3, got %d" % nf)
    if nv + nf > 2 ** 31 - 2:
        raise ValueError("faces: %d vertices and %d faces, together at most 2^31 - 2 (a centre is "
                         "a vertex)" % (nv, nf))
    check_face_indices(f, nv)
    if nv == 0 or nf == 0:
        return (v.copy(), f.copy(), np.zeros(0, np.int32), dict.fromkeys(COUNTS, 0))
    new_vertices, new_faces, source, counts = mesh_fill_holes(v, f, max_edges)
    stats = {name: int(c) for name, c in zip(COUNTS, counts)}
    return (np.concatenate([v, np.asarray(new_vertices, np.float32).reshape(-1, 3)]),
            np.concatenate([f, np.asarray(new_faces, np.int32).reshape(-1, 3)]),
            np.ascontiguousarray(source, np.int32).reshape(-1), stats)
