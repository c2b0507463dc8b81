"""Taubin smoothing of a surface mesh: the vertices move towards the mean of their neighbours
(a step with lambda) and back (a step with mu < -lambda), so that the terraces of an iso-surface
and the noise of a fused one flatten while the surface keeps its size.

The steps are two HIP kernels (csrc/raynet_smooth.inl; the definition is in include/raynet_hip.h at
rn_mesh_smooth): a gather over the corner table that the vertex normals use, in fp64, to the bit.
Here is the plumbing: the corner table (`appearance.corner_table`), the mask of the vertices on the
mesh's border (`boundary_vertices`: one sort of the edge keys and their run lengths), which are
pinned unless the caller says otherwise -- at an open border the umbrella operator is lopsided and
would pull the border inwards.

There is no CPU route: without a GPU `smooth_vertices` raises RaynetHipError.
"""
import math

import numpy as np
import torch

from . import _lib
from .appearance import _context, _dev, check_face_indices, corner_table, faces_tensor

MAX_ITERATIONS = 10000


def boundary_vertices(faces, n_vertices):
    """faces (nf, 3) of vertex indices (tensor on any device, or array) -> [nv] bool tensor on the
    faces' device: the vertices on an edge that lies in exactly one face.  An edge is the
    undirected pair of two different vertices of a face; a face with an index outside [0, nv) has
    no edges."""
    nv = int(n_vertices)
    f = faces_tensor(faces).to(torch.int64)
    f = f[((f >= 0) & (f < nv)).all(1)]
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    keys = (lo * nv + hi)[lo != hi]
    keys = torch.sort(keys).values
    edges, counts = torch.unique_consecutive(keys, return_counts=True)      # the run lengths
    single = edges[counts == 1]
    mask = torch.zeros((nv,), dtype=torch.bool, device=f.device)
    if nv:
        mask[single // nv] = True
        mask[single % nv] = True
    return mask


def check_parameters(iterations, lam, mu, max_move):
    """ValueError, naming the argument, for what rn_mesh_smooth would refuse."""
    if int(iterations) != iterations or not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError("iterations: a whole number in 0..%d, got %r" % (MAX_ITERATIONS, iterations))
    if not (math.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError("lam: in (0, 1], got %r" % (lam,))
    if not (math.isfinite(mu) and -1.0 <= mu <= 0.0):
        raise ValueError("mu: in [-1, 0], got %r" % (mu,))
    if not max_move > 0.0:
        raise ValueError("max_move: positive (inf or None: no limit), got %r" % (max_move,))


def mesh_smooth(vertices, faces, fixed, iterations, lam, mu, max_move):
    """The GPU call of `smooth_vertices`: host arrays vertices (nv, 3) float32, faces (nf, 3)
    int32 with every index in [0, nv), fixed [nv] bool or None -> (nv, 3) float32."""
    ctx = _context()
    v = _dev(vertices, torch.float32, ctx.device).reshape(-1, 3)
    f = _dev(faces, torch.int32, ctx.device).reshape(-1, 3)
    pinned = None if fixed is None else _dev(np.asarray(fixed, np.uint8), torch.uint8, ctx.device)
    with torch.cuda.device(ctx.device):
        offsets, corners = corner_table(f, len(v))
        out = ctx.mesh_smooth(v, f, offsets, corners, pinned, int(iterations), float(lam),
                              float(mu), float(max_move))
        return out.cpu().numpy()


def smooth_vertices(vertices, faces, iterations=10, lam=0.5, mu=-0.53, fixed="boundary",
                    max_move=None):
    """-> (nv, 3) float32: the vertices of the mesh (vertices (nv, 3), faces (nf, 3)) after
    `iterations` Taubin iterations -- a step p += lam (mean of the neighbours - p), then the same
    step with `mu` (negative; 0: plain Laplacian smoothing, which shrinks).  Every face around a
    vertex gives its two other vertices, so on a closed manifold every neighbour counts twice: the
    uniform umbrella.  fixed: "boundary" pins the vertices of `boundary_vertices`, None pins
    nothing, a mask over the vertices pins those; a vertex in no face never moves.  max_move: no
    coordinate ends farther than this from where it started (None: no limit)."""
    max_move = float("inf") if max_move is None else float(max_move)
    check_parameters(iterations, float(lam), float(mu), max_move)
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int32)
    nv = len(v)
    check_face_indices(f, nv)
    if fixed is None:
        pinned = None
    elif isinstance(fixed, str):
        if fixed != "boundary":
            raise ValueError('fixed: "boundary", None or a mask over the vertices, got %r' % (fixed,))
        device = "cuda" if torch.cuda.is_available() else "cpu"
        pinned = boundary_vertices(torch.from_numpy(f).to(device), nv).cpu().numpy()
    else:
        pinned = np.asarray(fixed)
        if pinned.shape != (nv,):
            raise ValueError("fixed: a mask over the vertices has %d entries, got %s"
                             % (nv, pinned.shape))
        pinned = pinned != 0
    if nv == 0:
        return v.copy()
    out = mesh_smooth(v, f, pinned, int(iterations), float(lam), float(mu), max_move)
    return np.ascontiguousarray(out, dtype=np.float32).reshape(nv, 3)
