"""A texture atlas for a surface mesh: the photographs baked per texel, and the lookup behind a
render.

Vertex colours keep one sample per vertex; after `--simplify` a vertex stands for a cell of
several voxels while the photographs resolve several pixels inside it.  The atlas gives every face
a chart of its own -- a right triangle of T texel steps per leg, two faces per square cell, with a
gutter so that a bilinear lookup never reads a neighbour's texel -- and `bake_texture` fills every
texel from the views that see its point of the face, with rn_project_colors's tests and weights
(include/raynet_hip.h, rn_texture_bake; csrc/raynet_texture.inl).  `sample_texture` turns the face
and barycentric planes of a render into colours (rn_texture_sample).

The layout is integer arithmetic (csrc/raynet_texture_args.h, restated here for the host side:
the UVs of a file, the atlas's size).  There is no CPU route: without a GPU `bake_texture` and
`sample_texture` raise RaynetHipError.
"""
import collections

import numpy as np
import torch

from .appearance import MAX_VIEWS, MODES, _context, _dev, pack_cameras, to_rgb8

MIN_T, MAX_T = 1, 1024
MARGIN = 5
MAX_EXTENT = 16384

AtlasLayout = collections.namedtuple("AtlasLayout", "n_faces T S cells_per_row cells rows Wt Ht")


def atlas_layout(n_faces, T, cells_per_row=None):
    """-> AtlasLayout of `n_faces` charts of T texel steps per leg: cells of S = T + 5 texels, two
    faces each, cells_per_row of them per row (default: the smallest Cw with Cw Cw >= cells), Wt x
    Ht texels."""
    n_faces, T = int(n_faces), int(T)
    if n_faces < 0 or not MIN_T <= T <= MAX_T:
        raise ValueError("atlas: n_faces >= 0 and T in %d..%d, got %d and %d"
                         % (MIN_T, MAX_T, n_faces, T))
    cells = (n_faces + 1) // 2
    if cells_per_row is None:
        cells_per_row = max(1, int(np.sqrt(cells)))
        while cells_per_row * cells_per_row < cells:            # (whole numbers decide)
            cells_per_row += 1
        while cells_per_row > 1 and (cells_per_row - 1) * (cells_per_row - 1) >= cells:
            cells_per_row -= 1
    Cw = int(cells_per_row)
    if Cw < 1:
        raise ValueError("atlas: cells_per_row >= 1, got %d" % Cw)
    S = T + MARGIN
    rows = (cells + Cw - 1) // Cw
    if cells and max(Cw * S, rows * S) > MAX_EXTENT:
        raise ValueError("atlas: %d faces at T = %d need %d x %d texels, more than %d a side"
                         % (n_faces, T, Cw * S, rows * S, MAX_EXTENT))
    return AtlasLayout(n_faces, T, S, Cw, cells, rows, Cw * S, rows * S)


def face_corners(layout):
    """(nf, 3, 2) int64: the texels (x, y) of the corners p0, p1, p2 of every face's chart."""
    T, S, Cw = layout.T, layout.S, layout.cells_per_row
    f = np.arange(layout.n_faces, dtype=np.int64)
    x, y = (f // 2 % Cw * S)[:, None], (f // 2 // Cw * S)[:, None]
    lower = (f % 2 == 0)[:, None]
    a = np.where(lower, np.array([1, T + 1, 1]), np.array([T + 3, 3, T + 3]))
    b = np.where(lower, np.array([1, 1, T + 1]), np.array([T + 3, T + 3, 3]))
    return np.stack([x + a, y + b], -1)


def face_uvs(n_faces, layout):
    """(nf, 3, 2) float64: the texture coordinates of every face's three corners as files carry
    them, ((x + 0.5) / Wt, 1 - (y + 0.5) / Ht): texel centres, v upwards."""
    if int(n_faces) != layout.n_faces:
        raise ValueError("%d faces for a layout of %d" % (n_faces, layout.n_faces))
    c = face_corners(layout).astype(np.float64)
    return np.stack([(c[..., 0] + 0.5) / max(layout.Wt, 1),
                     1.0 - (c[..., 1] + 0.5) / max(layout.Ht, 1)], -1)


def owned_texels(layout):
    """(Ht, Wt) bool: the texels some face owns."""
    ty, tx = np.mgrid[0:layout.Ht, 0:layout.Wt]
    S = layout.S
    lower = tx % S + ty % S <= layout.T + 3
    f = 2 * (ty // S * layout.cells_per_row + tx // S) + np.where(lower, 0, 1)
    return f < layout.n_faces


class MeshTexture(object):
    """What `bake_texture` returns: device tensors texture (Ht, Wt, C) float32 in the images'
    range, weight (Ht, Wt) float32 and views (Ht, Wt) int32 (the bits of the mask: bit k, view k
    counted), and the `layout`."""
    __slots__ = ("texture", "weight", "views", "layout")

    def __init__(self, texture, weight, views, layout):
        self.texture, self.weight, self.views, self.layout = texture, weight, views, layout

    def filled(self, unseen=(0.5, 0.5, 0.5)):
        """(Ht, Wt, C) float32 host array: the texture with `unseen` (its first C values; grey
        from the first for one channel) at the texels a face owns that no view saw."""
        out = self.texture.cpu().numpy().copy()
        hole = (self.views.cpu().numpy() == 0) & owned_texels(self.layout)
        out[hole] = np.asarray(unseen, np.float32)[:out.shape[2]]
        return out

    def with_unseen(self, unseen=(0.5, 0.5, 0.5)):
        """-> a MeshTexture whose texture is `filled(unseen)`, on the device: what a lookup should
        read where no view saw the surface (vertex colours get the same grey)."""
        t = torch.from_numpy(self.filled(unseen)).to(self.texture.device)
        return MeshTexture(t, self.weight, self.views, self.layout)

    def rgb8(self, unseen=(0.5, 0.5, 0.5)):
        """(Ht, Wt, 3) uint8 of `filled`, by appearance.to_rgb8's rule."""
        t = self.filled(unseen)
        return to_rgb8(t.reshape(-1, t.shape[2])).reshape(t.shape[0], t.shape[1], 3)

    def save_png(self, path, unseen=(0.5, 0.5, 0.5)):
        """The atlas as an 8-bit PNG; row 0 of the atlas is the top row."""
        from PIL import Image
        Image.fromarray(self.rgb8(unseen)).save(path)


def bake_texture(mesh, cameras, images, T, depth_maps=None, tol=0.0, min_cos=0.0, border=0.0,
                 mode="blend", normals="face"):
    """The photographs baked into an atlas of `mesh` (volume.SurfaceMesh) -> MeshTexture.

    cameras, images, depth_maps, tol, min_cos, border and mode are appearance.project_colors's;
    every texel is a point of its face.  normals "face": a texel faces a view with its face's
    normal; "vertex": with the mesh's vertex normals interpolated (computed if absent)."""
    if mode not in MODES:
        raise ValueError("mode: one of %s, got %r" % (", ".join(sorted(MODES)), mode))
    if normals not in ("face", "vertex"):
        raise ValueError("normals: 'face' or 'vertex', got %r" % (normals,))
    if mesh.empty:
        raise ValueError("the mesh is empty: there is no surface to texture")
    cameras = list(cameras)
    V = len(cameras)
    if V > MAX_VIEWS:
        raise ValueError("%d views: at most %d per call (a bit of the mask each) -- choose the "
                         "frames that see the surface best" % (V, MAX_VIEWS))
    if len(images) != V or (depth_maps is not None and len(depth_maps) != V):
        raise ValueError("%d cameras, %d images and %s depth maps" % (
            V, len(images), "no" if depth_maps is None else len(depth_maps)))
    if V == 0:
        raise ValueError("no view to take colours from")
    layout = atlas_layout(len(mesh.faces), T)
    ctx = _context("textures")
    dev = ctx.device
    stack = np.stack([np.asarray(i, np.float32) for i in images])
    if stack.ndim == 3:
        stack = stack[..., None]
    if stack.ndim != 4 or not 1 <= stack.shape[3] <= 4:
        raise ValueError("images: (H, W) or (H, W, C <= 4) arrays of one shape, got %s"
                         % (stack.shape[1:],))
    H, W, C = stack.shape[1:]
    depths = None
    if depth_maps is not None:
        depths = torch.stack([_dev(d, torch.float32, dev) for d in depth_maps])
        if tuple(depths.shape) != (V, H, W):
            raise ValueError("depth maps %s for images of %s" % (tuple(depths.shape[1:]), (H, W)))
    nrm = None
    if normals == "vertex":
        if mesh.normals is None:
            mesh.compute_normals()
        nrm = _dev(mesh.normals, torch.float32, dev).reshape(-1, 3)
    texture = torch.empty((layout.Ht, layout.Wt, C), dtype=torch.float32, device=dev)
    weight = torch.empty((layout.Ht, layout.Wt), dtype=torch.float32, device=dev)
    views = torch.empty((layout.Ht, layout.Wt), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ctx.texture_bake(_dev(mesh.vertices, torch.float32, dev).reshape(-1, 3),
                         _dev(mesh.faces, torch.int32, dev).reshape(-1, 3), nrm, layout.T,
                         layout.cells_per_row, _dev(pack_cameras(cameras), torch.float64, dev),
                         _dev(stack, torch.float32, dev), depths, tol, min_cos, border, MODES[mode],
                         texture, weight, views)
    return MeshTexture(texture, weight, views, layout)


def sample_texture(render, texture, bilinear=True):
    """(V, H, W, C) float32 device tensor: `texture` (MeshTexture) looked up at every pixel of
    `render` (render.MeshRender) by its face and barycentrics; 0 where a ray hits nothing."""
    ctx = _context("textures")
    face = render.face.contiguous()
    C = int(texture.texture.shape[2])
    color = torch.empty(tuple(face.shape) + (C,), dtype=torch.float32, device=face.device)
    with torch.cuda.device(face.device):
        ctx.texture_sample(face, render.bary.contiguous(), texture.layout.n_faces, texture.layout.T,
                           texture.layout.cells_per_row, texture.texture, bilinear, color)
    return color
