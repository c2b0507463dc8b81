"""What a reconstruction looks like: vertex normals of a mesh and the colours the scene's images
give to a mesh's vertices or a cloud's points.

The work is two HIP kernels (csrc/raynet_appearance.inl; the definitions are in
include/raynet_hip.h at rn_vertex_area_normals / rn_project_colors).  Here is the plumbing: the
mesh's corner table by vertex (one stable sort, a bincount and a cumsum), the cameras packed as
rows of 15 float64 (P row-major | centre), one upload of the stacked images and depth maps.

There is no CPU route: without a GPU the functions raise RaynetHipError.
"""
import numpy as np
import torch

from . import _lib

MAX_VIEWS = 32
MODES = {"blend": 0, "best": 1}


class ProjectedColors(object):
    """What `project_colors` returns, as host arrays: colors (n, C) float32 in the images' range,
    weight [n] float32 (the sum of the counted views' cos^2, or their number without normals) and
    views [n] uint32 (bit v: view v counted)."""
    __slots__ = ("colors", "weight", "views")

    def __init__(self, colors, weight, views):
        self.colors, self.weight, self.views = colors, weight, views

    @property
    def seen(self):
        return self.views != 0


def _context(work="colours"):
    if not torch.cuda.is_available():
        raise _lib.RaynetHipError(
            "no GPU visible: raynet_amd %s on MI355X only (no CPU fallback)" % work)
    from .hip_implementations import get_context
    return get_context()


def _tensor(x):
    return x.detach() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def _dev(x, dtype, device):
    return _tensor(x).to(device=device, dtype=dtype).contiguous()


def faces_tensor(faces):
    """faces (nf, 3) of vertex indices, a tensor on any device or an array -> an (nf, 3) tensor on
    the faces' device, with their dtype."""
    return _tensor(faces).reshape(-1, 3)


def check_face_indices(faces, n_vertices):
    """ValueError for faces (tensor or array) with an index outside the n_vertices vertices."""
    if len(faces) and (int(faces.min()) < 0 or int(faces.max()) >= n_vertices):
        raise ValueError("faces: a vertex index outside 0..%d" % (n_vertices - 1))


def corner_table(faces, n_vertices):
    """faces (nf, 3) int32 device tensor -> (offsets [nv + 1] i32, corners [3 nf] i32): the
    indices c = 3 face + slot of the flattened faces sorted by the vertex they name, ascending c
    within a vertex, and the exclusive prefix of the vertices' corner counts."""
    flat = faces.reshape(-1).to(torch.int64)
    corners = torch.sort(flat, stable=True).indices.to(torch.int32)
    counts = torch.bincount(flat, minlength=int(n_vertices))
    offsets = torch.zeros((int(n_vertices) + 1,), dtype=torch.int64, device=faces.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets.to(torch.int32).contiguous(), corners.contiguous()


def pack_cameras(cameras):
    """[V, 15] float64: Camera.P (3 x 4, row-major) | Camera.center[:3] per row."""
    rows = np.empty((len(cameras), 15), np.float64)
    for row, cam in zip(rows, cameras):
        row[:12] = np.asarray(cam.P, np.float64).reshape(12)
        row[12:] = np.asarray(cam.center, np.float64).reshape(-1)[:3]
    return rows


def normalized(normals):
    """Unit vectors of float32 rows, computed in float64; a zero vector stays zero."""
    n = np.asarray(normals, np.float32).astype(np.float64)
    length = np.sqrt((n * n).sum(1, keepdims=True))
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0).astype(np.float32)


def vertex_normals(vertices, faces, unit=True):
    """(nv, 3) float32 normals of an indexed triangle mesh (vertices (nv, 3), faces (nf, 3)): the
    sum of the area-weighted normals e1 x e2 of the faces around every vertex, pointing where the
    faces' counter-clockwise side points.  unit: divided by their length (a zero vector -- a
    vertex in no face, or in faces whose areas cancel -- stays zero); else twice the area around
    the vertex long."""
    ctx = _context()
    v = _dev(vertices, torch.float32, ctx.device).reshape(-1, 3)
    f = _dev(faces, torch.int32, ctx.device).reshape(-1, 3)
    check_face_indices(f, len(v))
    offsets, corners = corner_table(f, len(v))
    normals = ctx.vertex_area_normals(v, f, offsets, corners).cpu().numpy()
    return normalized(normals) if unit else normals


def project_colors(points, cameras, images, depth_maps=None, normals=None, tol=0.0, min_cos=0.0,
                   border=0.0, mode="blend"):
    """Colours of `points` (n, 3) from the views that see them -> ProjectedColors.

    cameras: common.camera.Camera objects (P, center); images: one (H, W, C) or (H, W) float
    array per camera, all of one shape, C <= 4; depth_maps: one (H, W) map per camera of distances
    to the camera centre, the occluders -- a view sees a point no farther than its map's value at
    the point's pixel plus `tol` (scene units); None: nothing occludes.  normals (n, 3): a view
    sees only points that face it (cos > min_cos) and weighs in with cos^2; a zero normal faces
    everything with weight 1.  border: pixels to stay away from the image's edge.  mode "blend":
    the weighted mean of the views, "best": the view with the largest weight, the first of
    equals."""
    if mode not in MODES:
        raise ValueError("mode: one of %s, got %r" % (", ".join(sorted(MODES)), mode))
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
    ctx = _context()
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
    p = _dev(points, torch.float32, dev).reshape(-1, 3)
    nrm = None
    if normals is not None:
        nrm = _dev(normals, torch.float32, dev).reshape(-1, 3)
        if len(nrm) != len(p):
            raise ValueError("%d normals for %d points" % (len(nrm), len(p)))
    n = len(p)
    colors = torch.empty((n, C), dtype=torch.float32, device=dev)
    weight = torch.empty((n,), dtype=torch.float32, device=dev)
    views = torch.empty((n,), dtype=torch.int32, device=dev)
    ctx.project_colors(p, nrm, _dev(pack_cameras(cameras), torch.float64, dev),
                       _dev(stack, torch.float32, dev), depths, tol, min_cos, border, MODES[mode],
                       colors, weight, views)
    return ProjectedColors(colors.cpu().numpy(), weight.cpu().numpy(),
                           views.cpu().numpy().view(np.uint32))


def to_rgb8(colors, seen=None, unseen=(0.5, 0.5, 0.5)):
    """(n, C) float colours -> (n, 3) uint8, rint(clip(c, 0, 1) * 255): one channel gives grey,
    two give grey from the first, the fourth of four is dropped; rows where `seen` is False get
    `unseen`."""
    c = np.asarray(colors, np.float32)
    c = c.reshape(len(c), -1)
    rgb = c[:, :3] if c.shape[1] >= 3 else np.repeat(c[:, :1], 3, axis=1)
    rgb = np.array(rgb, np.float32)
    if seen is not None:
        rgb[~np.asarray(seen, bool)] = np.asarray(unseen, np.float32)
    return np.rint(np.clip(rgb, 0.0, 1.0) * np.float32(255)).astype(np.uint8)


def scene_views(scene, frame_idxs):
    """(cameras, images) of the frames of a scene; a frame without pixels is an error."""
    frame_idxs = [int(i) for i in frame_idxs]
    if len(frame_idxs) > MAX_VIEWS:
        raise ValueError("%d frames: at most %d views per call -- choose the frames that see the "
                         "surface best" % (len(frame_idxs), MAX_VIEWS))
    frames = [scene.get_image(i) for i in frame_idxs]
    for i, f in zip(frame_idxs, frames):
        if getattr(f, "image", None) is None:
            raise ValueError("frame %d of the scene has no image to take colours from" % i)
    return [f.camera for f in frames], [f.image for f in frames]
