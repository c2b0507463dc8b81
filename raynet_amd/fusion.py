"""Depth maps fused into a surface: a truncated signed distance volume over the scene's grid and
the triangle mesh of its zero level.

The depth maps of a pass -- of any factory, with or without an MRF -- or a scene's ground-truth
maps go into one HIP kernel (csrc/raynet_fusion.inl; the definition is in include/raynet_hip.h at
rn_tsdf_integrate): every voxel takes the weighted mean, over the views that see it, of its signed
distance to the surface each view recorded, truncated to `trunc`.  `TSDFVolume.mesh()` is the zero
level of that field by the package's marching tetrahedra (HipContext.isosurface), a `SurfaceMesh`
like the one of an `OccupancyVolume`: it saves, ray-casts, samples, shades and colours the same.

There is no CPU route: without a GPU the functions raise RaynetHipError.
"""
import numpy as np
import torch

from . import _lib
from .appearance import pack_cameras
from .common.scene import get_voxel_grid
from .volume import SurfaceMesh


def _grid_context(bbox, grid_shape):
    """The context of a grid, as OccupancyVolume._context obtains it."""
    if not torch.cuda.is_available():
        raise _lib.RaynetHipError(
            "no GPU visible: raynet_amd fuses depth maps on MI355X only (no CPU fallback)")
    from .hip_implementations import get_context
    from .volume import MAX_M
    ctx = get_context(M=min(sum(grid_shape), MAX_M), H=1, W=1, bbox=bbox, grid_shape=grid_shape)
    if not ctx._grid_set:
        ctx.set_voxel_grid(np.ascontiguousarray(
            get_voxel_grid(bbox, grid_shape).transpose(1, 2, 3, 0)))
    return ctx


def _stack(maps, device, what):
    maps = [m.detach() if isinstance(m, torch.Tensor) else
            torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)) for m in maps]
    stack = torch.stack([m.to(device=device, dtype=torch.float32) for m in maps]).contiguous()
    if stack.dim() != 3:
        raise ValueError("%s: (H, W) maps of one shape, got %s" % (what, tuple(stack.shape[1:])))
    return stack


class TSDFVolume(object):
    """tsdf, weight: [gx][gy][gz] float32 (array or tensor, host or device) -- the weighted mean
    of the views' signed distances to the surface in units of `trunc` (positive in front of it, 1
    in free space and where no view counts) and the sum of the weights of the views that count (0:
    unobserved); bbox: the 6 numbers of the scene's bounding box; grid_shape: (gx, gy, gz);
    trunc: the truncation distance in scene units."""

    KEYS = ("tsdf", "weight", "bbox", "grid_shape", "trunc")

    def __init__(self, tsdf, weight, bbox, grid_shape, trunc):
        self.grid_shape = tuple(int(g) for g in np.asarray(grid_shape).ravel())
        if len(self.grid_shape) != 3 or min(self.grid_shape) < 1:
            raise ValueError("grid_shape: three positive sizes, got %r" % (grid_shape,))
        self.bbox = np.ascontiguousarray(np.asarray(bbox, dtype=np.float32).reshape(-1))
        if self.bbox.shape != (6,):
            raise ValueError("bbox: 6 numbers, got %r" % (bbox,))
        self.trunc = float(np.asarray(trunc).reshape(()))
        if not (self.trunc > 0.0 and np.isfinite(self.trunc)):
            raise ValueError("trunc: a positive distance, got %r" % (trunc,))
        self.tsdf = self._grid(tsdf, "tsdf")
        self.weight = self._grid(weight, "weight")

    def _grid(self, t, name):
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
        if t.dtype != torch.float32 or tuple(t.shape) != self.grid_shape:
            raise ValueError("%s: expected float32 of shape %s, got %s of shape %s"
                             % (name, self.grid_shape, t.dtype, tuple(t.shape)))
        return t.contiguous()

    # ---- file ------------------------------------------------------------------------------
    def save(self, path):
        """An .npz of `tsdf` and `weight` [gx][gy][gz] f32, `bbox` [6] f32, `grid_shape` [3] i32
        and `trunc` f64."""
        with open(path, "wb") as f:        # (a file object: savez appends no suffix of its own)
            np.savez(f, tsdf=self.tsdf.cpu().numpy(), weight=self.weight.cpu().numpy(),
                     bbox=self.bbox, grid_shape=np.array(self.grid_shape, dtype=np.int32),
                     trunc=np.array(self.trunc, dtype=np.float64))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if sorted(z.files) != sorted(cls.KEYS):
                raise ValueError("%s: expected the arrays %s, found %s"
                                 % (path, ", ".join(cls.KEYS), ", ".join(sorted(z.files))))
            return cls(z["tsdf"], z["weight"], z["bbox"], z["grid_shape"], z["trunc"])

    # ---- the surface ------------------------------------------------------------------------
    def field(self, min_weight=0.0):
        """[gx][gy][gz] float32: -tsdf where the voxel was observed (weight > 0 and weight >=
        min_weight), NaN elsewhere; its zero level is the surface, its positive side the inside."""
        observed = (self.weight > 0) & (self.weight >= float(min_weight))
        return torch.where(observed, -self.tsdf, torch.full_like(self.tsdf, float("nan")))

    def mesh(self, min_weight=0.0):
        """-> SurfaceMesh: the zero level of the fused distances, interpolated between the voxel
        centres (marching tetrahedra, HipContext.isosurface on `field(min_weight)` at 0, not
        closed): behind the surface is inside, the normals point into free space.

        A tetrahedron with an unobserved corner contributes no face: every face a tetrahedron
        produces has a vertex on each of its inside-outside edges, an unobserved corner is NaN,
        which counts as outside, and an edge to a NaN corner gives a NaN vertex -- and the faces
        with such a vertex are dropped (SurfaceMesh.without_nonfinite).  So the mesh is open where
        observation ends, and the shell that would otherwise appear `trunc` behind the surface,
        where observed voxels meet unobserved ones, is gone."""
        if not min_weight >= 0.0:
            raise ValueError("min_weight: 0 or more, got %r" % (min_weight,))
        ctx = _grid_context(self.bbox, self.grid_shape)
        vertices, faces = ctx.isosurface(self.field(min_weight).to(ctx.device), 0.0, closed=False)
        return SurfaceMesh(vertices, faces).without_nonfinite()


def fuse_depth_maps(depth_maps, cameras, bbox, grid_shape, trunc=None, weights=None, border=0.0):
    """One (H, W) map of distances to the camera centre per camera (common.camera.Camera: P,
    center), all of one shape, fused over the grid `grid_shape` of the box `bbox` -> TSDFVolume.

    A pixel that is 0, negative, NaN or +inf holds no measurement.  weights: one (H, W) map per
    camera, e.g. the confidence of `forward_pass(..., with_statistics=True)`; a pixel whose weight
    is 0, negative, NaN or +inf does not count; None: every measurement weighs 1.  trunc: the
    truncation distance in scene units, None: three times the largest voxel side.  border: pixels
    to stay away from the image's edge."""
    cameras, depth_maps = list(cameras), list(depth_maps)
    if len(depth_maps) != len(cameras) or (weights is not None and len(weights) != len(cameras)):
        raise ValueError("%d cameras, %d depth maps and %s weight maps" % (
            len(cameras), len(depth_maps), "no" if weights is None else len(weights)))
    if not cameras:
        raise ValueError("no depth map to fuse")
    grid_shape = tuple(int(g) for g in np.asarray(grid_shape).ravel())
    bbox = np.asarray(bbox, dtype=np.float32).reshape(-1)
    if trunc is None:
        extent = bbox[3:].astype(np.float64) - bbox[:3].astype(np.float64)
        trunc = 3.0 * float((extent / np.array(grid_shape, np.float64)).max())
    ctx = _grid_context(bbox, grid_shape)
    depths = _stack(depth_maps, ctx.device, "depth_maps")
    if weights is not None:
        weights = _stack(weights, ctx.device, "weights")
        if weights.shape != depths.shape:
            raise ValueError("weights %s for depth maps of %s"
                             % (tuple(weights.shape[1:]), tuple(depths.shape[1:])))
    rows = torch.from_numpy(pack_cameras(cameras)).to(ctx.device)
    tsdf, weight = ctx.tsdf_integrate(rows, depths, weights, trunc, border)
    return TSDFVolume(tsdf, weight, bbox, grid_shape, trunc)


def fuse_scene(scene, depth_maps, frame_idxs, grid_shape, trunc=None, weights=None, border=0.0):
    """`fuse_depth_maps` with the cameras of the scene's frames `frame_idxs` and the scene's
    bounding box; depth_maps (and weights): one map per frame, in that order."""
    frame_idxs = [int(i) for i in frame_idxs]
    cameras = [scene.get_image(i).camera for i in frame_idxs]
    return fuse_depth_maps(depth_maps, cameras, np.asarray(scene.bbox).reshape(-1), grid_shape,
                           trunc=trunc, weights=weights, border=border)
