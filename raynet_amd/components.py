"""The connected components of a surface mesh: which piece every vertex and face belongs to, how
large the pieces are, and which of them to keep.

What comes out of the marching tetrahedra on real predictions is one surface plus debris: small
closed shells around isolated blobs of belief, shreds of TSDF surface around a noisy depth pixel.
The labels are a lock-free union-find on the GPU (csrc/raynet_components.inl; the definition is in
include/raynet_hip.h at rn_mesh_components): two vertices are connected if a face names both --
positions play no part, so two pieces that touch only in space, with duplicated vertex rows, are
two components; the package's iso-surfaces share one vertex per lattice edge, so for them
"connected" is what one expects.  Here is the plumbing: dense ids, sizes, the selection
(`MeshComponents.select`) and the compaction of a mesh (`keep_faces`), all masks and gathers.

There is no CPU route: without a GPU `mesh_components` raises RaynetHipError.
"""
import numpy as np
import torch

from .appearance import _context, _dev


class MeshComponents(object):
    """The components of a mesh of nv vertices, as host arrays, in the order of their smallest
    vertex:
      labels      (nv,) int32  the smallest vertex index of every vertex's component
      roots       (K,)  int32  the labels that occur, ascending
      component   (nv,) int32  the dense id of every vertex's component: roots[component] == labels
      n_vertices  (K,)  int64  vertices per component
      n_faces     (K,)  int64  faces per component (a vertex in no face is a component of 0 faces)
    """

    def __init__(self, labels, vertex_counts, face_counts):
        self.labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        nv = len(self.labels)
        vertex_counts = np.asarray(vertex_counts).reshape(-1)
        face_counts = np.asarray(face_counts).reshape(-1)
        if len(vertex_counts) != nv or len(face_counts) != nv:
            raise ValueError("labels, vertex_counts and face_counts: one entry per vertex, got "
                             "%d, %d, %d" % (nv, len(vertex_counts), len(face_counts)))
        is_root = self.labels == np.arange(nv, dtype=np.int32)
        self.roots = np.flatnonzero(is_root).astype(np.int32)
        dense = np.cumsum(is_root) - 1                      # the id of a root, at the root
        self.component = dense[self.labels].astype(np.int32) if nv else np.zeros(0, np.int32)
        self.n_vertices = vertex_counts[self.roots].astype(np.int64)
        self.n_faces = face_counts[self.roots].astype(np.int64)

    def __len__(self):
        return len(self.roots)

    def face_component(self, faces):
        """(nf,) int32: the dense id of every face's component (its first vertex's); -1 for a
        face with an index outside [0, nv), which belongs to no component."""
        faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
        counted = ((faces >= 0) & (faces < len(self.labels))).all(1)
        out = np.full(len(faces), -1, dtype=np.int32)
        out[counted] = self.component[faces[counted, 0]]
        return out

    def face_mask(self, faces, keep):
        """(nf,) bool: the faces of the components of `keep` ((K,) bool); never a face that belongs
        to no component."""
        of = self.face_component(faces)
        keep = np.asarray(keep, dtype=bool)
        return (of >= 0) & keep[np.maximum(of, 0)] if len(keep) else np.zeros(len(of), dtype=bool)

    def largest(self, k):
        """The ids of the k components with the most faces, descending, ties to the lower id."""
        order = np.argsort(-self.n_faces, kind="stable")
        return order[:max(int(k), 0)]

    def select(self, min_faces=None, min_fraction=None, keep_largest=None):
        """(K,) bool: the components that meet every criterion given -- at least `min_faces`
        faces; at least `min_fraction` of the largest component's faces (n_faces >= min_fraction *
        max, in float64); among the `keep_largest` largest.  A component with 0 faces is never
        selected."""
        keep = self.n_faces > 0
        if min_faces is not None:
            keep &= self.n_faces >= int(min_faces)
        if min_fraction is not None and len(self.n_faces):
            keep &= self.n_faces.astype(np.float64) >= \
                np.float64(min_fraction) * np.float64(self.n_faces.max())
        if keep_largest is not None:
            top = np.zeros(len(self.n_faces), dtype=bool)
            top[self.largest(keep_largest)] = True
            keep &= top
        return keep


def check_criteria(min_faces=None, min_fraction=None, keep_largest=None):
    """ValueError unless at least one criterion is given and each is in its range."""
    if min_faces is None and min_fraction is None and keep_largest is None:
        raise ValueError("no criterion: give min_faces, min_fraction or keep_largest")
    if min_faces is not None and int(min_faces) < 1:
        raise ValueError("min_faces: 1 or more, got %r" % (min_faces,))
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError("keep_largest: 1 or more, got %r" % (keep_largest,))
    if min_fraction is not None and not 0.0 < float(min_fraction) <= 1.0:
        raise ValueError("min_fraction: in (0, 1], got %r" % (min_fraction,))


def mesh_components(faces, n_vertices):
    """faces (nf, 3) of vertex indices (array or tensor, host or device) of a mesh with
    `n_vertices` vertices -> MeshComponents.  A face with an index outside [0, n_vertices)
    connects nothing and is counted nowhere."""
    ctx = _context("labels components")
    f = _dev(faces, torch.int32, ctx.device).reshape(-1, 3)
    with torch.cuda.device(ctx.device):
        labels, vertex_counts, face_counts = ctx.mesh_components(f, int(n_vertices))
    return MeshComponents(labels.cpu().numpy(), vertex_counts.cpu().numpy(),
                          face_counts.cpu().numpy())


def keep_faces(mesh, mask):
    """-> a new SurfaceMesh of the faces of `mask` ((nf,) bool) and the vertices they name,
    renumbered; the order of both is kept, normals and colours go along."""
    from .volume import SurfaceMesh
    faces = torch.from_numpy(mesh.faces).long()[torch.from_numpy(np.asarray(mask, dtype=bool))]
    used = torch.zeros(len(mesh.vertices), dtype=torch.bool)
    used[faces.reshape(-1)] = True
    new = torch.cumsum(used, 0) - 1
    keep = used.numpy()
    return SurfaceMesh(mesh.vertices[keep], new[faces].to(torch.int32).numpy(),
                       None if mesh.normals is None else mesh.normals[keep],
                       None if mesh.colors is None else mesh.colors[keep])


def filter_small(mesh, min_faces=None, min_fraction=None, keep_largest=None):
    """SurfaceMesh.without_small_components with its tally -> (the new mesh, the number of
    components found, the number kept).  An empty mesh stays empty, without the GPU."""
    check_criteria(min_faces, min_fraction, keep_largest)
    if mesh.empty:
        return keep_faces(mesh, np.zeros(0, dtype=bool)), 0, 0
    found = mesh.components()
    keep = found.select(min_faces, min_fraction, keep_largest)
    return keep_faces(mesh, found.face_mask(mesh.faces, keep)), len(found), int(keep.sum())
