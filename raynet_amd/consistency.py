"""Do the other views confirm a depth or contradict it?  The cross-view check of points and depth
maps.

Every point goes through one HIP kernel (csrc/raynet_consistency.inl; the definition is in
include/raynet_hip.h at rn_points_consistency): every view projects the point, reads the depth it
recorded at the nearest pixel and says one of three things -- it agrees (the point lies at that
depth, within tol_abs + tol_rel * depth), it is violated (it sees past the point: the point floats
in that view's free space), or it is merely occluded there (it recorded something nearer, which is
no contradiction).  The answers come back as bit masks, one bit per view, and the mean signed
distance over the agreeing views.  `check_points` asks about any cloud or mesh vertices,
`check_depth_maps` about every pixel of every map, each against all the other maps; a
`DepthConsistency` turns the masks into counts, a keep mask and a filtered map whose dropped
pixels are 0, "no measurement" to `fusion.fuse_depth_maps`.

The depth is read at the nearest pixel, not interpolated: a tolerance must exceed the depth step
of one pixel of the surfaces it is to confirm, or slanted surfaces violate themselves.

There is no CPU route: without a GPU the functions raise RaynetHipError.
"""
import collections

import numpy as np
import torch

from .appearance import _context, pack_cameras
from .fusion import _stack

MAX_VIEWS = 32

PointConsistency = collections.namedtuple("PointConsistency", "seen agree violate residual")
PointConsistency.__doc__ = """What `check_points` returns, as host arrays over the n points: seen,
agree, violate [n] uint32 (bit v: view v measures something at the point's pixel / agrees with the
point / sees past it; a view with its bit in `seen` alone is occluded there) and residual [n]
float32, the mean signed distance over the agreeing views (positive: the views place the surface
behind the point), 0 where none agrees."""


def popcount(mask):
    """The number of set bits of every uint32 of `mask`, as uint8."""
    m = np.ascontiguousarray(mask, np.uint32)
    return np.unpackbits(m.view(np.uint8).reshape(m.shape + (4,)), axis=-1).sum(-1, dtype=np.uint8)


def _views(cameras, depth_maps, device):
    """The camera rows and the stacked maps on the device, after the checks that need no GPU
    call."""
    V = len(cameras)
    if len(depth_maps) != V:
        raise ValueError("%d cameras and %d depth maps" % (V, len(depth_maps)))
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError("%d views: 1 to %d per call (a bit of the masks each)" % (V, MAX_VIEWS))
    depths = _stack(depth_maps, device, "depth_maps")
    return torch.from_numpy(pack_cameras(cameras)).to(device), depths


def _tolerances(tol_abs, tol_rel, border):
    for name, value in (("tol_abs", tol_abs), ("tol_rel", tol_rel), ("border", border)):
        if not (value >= 0.0 and np.isfinite(value)):
            raise ValueError("%s: a finite number that is 0 or more, got %r" % (name, value))


def check_points(points, cameras, depth_maps, exclude=-1, tol_abs=0.0, tol_rel=0.01, border=0.0):
    """What the views say about `points` (n, 3), a cloud's points or a mesh's vertices ->
    PointConsistency.

    cameras: common.camera.Camera objects (P, center), at most 32; depth_maps: one (H, W) map per
    camera of distances to the camera centre, all of one shape (0, a negative value, NaN and +inf
    are "no measurement").  exclude: the index of one view that is not asked (the view the points
    came from), -1: every view is.  A view agrees with a point whose signed distance to the depth
    it recorded lies within tol_abs + tol_rel * depth (scene units).  border: pixels to stay away
    from the maps' edge."""
    cameras, depth_maps = list(cameras), list(depth_maps)
    _tolerances(tol_abs, tol_rel, border)
    p = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points: expected shape (n, 3), got %s" % (p.shape,))
    ctx = _context("checks depth maps")
    rows, depths = _views(cameras, depth_maps, ctx.device)
    pts = torch.from_numpy(np.ascontiguousarray(p.T, dtype=np.float64)).to(ctx.device)
    seen, agree, violate, residual = ctx.points_consistency(pts, rows, depths, exclude, tol_abs,
                                                            tol_rel, border)
    return PointConsistency(seen.cpu().numpy().view(np.uint32), agree.cpu().numpy().view(np.uint32),
                            violate.cpu().numpy().view(np.uint32), residual.cpu().numpy())


class DepthConsistency(object):
    """What the other views say about every pixel of one depth map, as host arrays of the map's
    shape: seen, agree, violate (H, W) uint32 (bit v: view v of the call; the map's own view has
    no bit), residual (H, W) float32 and `measured` (H, W) bool, whether the pixel itself holds a
    measurement (0 < depth < inf)."""
    __slots__ = ("seen", "agree", "violate", "residual", "measured")

    def __init__(self, seen, agree, violate, residual, measured):
        self.seen, self.agree, self.violate = seen, agree, violate
        self.residual, self.measured = residual, measured

    @property
    def seen_count(self):
        return popcount(self.seen)

    @property
    def agree_count(self):
        return popcount(self.agree)

    @property
    def violate_count(self):
        return popcount(self.violate)

    def keep(self, min_views=2, max_violations=0):
        """(H, W) bool: the pixel holds a measurement, at least `min_views` other views agree with
        it and at most `max_violations` see past it."""
        if min_views < 0 or max_violations < 0:
            raise ValueError("min_views, max_violations: 0 or more, got %r, %r"
                             % (min_views, max_violations))
        return self.measured & (self.agree_count >= min_views) & \
            (self.violate_count <= max_violations)

    def filtered(self, depth, min_views=2, max_violations=0):
        """The (H, W) float32 map `depth` with 0 where the pixel is not kept: 0 is "no
        measurement" to rn_tsdf_integrate."""
        depth = np.asarray(depth.detach().cpu() if isinstance(depth, torch.Tensor) else depth,
                           np.float32)
        if depth.shape != self.measured.shape:
            raise ValueError("depth: expected the shape %s, got %s"
                             % (self.measured.shape, depth.shape))
        return np.where(self.keep(min_views, max_violations), depth, np.float32(0))


def check_depth_maps(depth_maps, cameras=None, P_pinvs=None, centers=None, scene=None,
                     frame_idxs=None, tol_abs=0.0, tol_rel=0.01, border=0.0):
    """Every pixel of every map against all the other maps -> one DepthConsistency per view.

    depth_maps: one (H, W) map of distances to the camera centre per view, all of one shape, at
    most 32.  The views are either `cameras` (objects with P and center; their back-projection is
    P_pinvs / centers where given -- one [4][3] matrix and one centre of 4 components per view --
    else the cameras' own P_pinv and center) or the frames `frame_idxs` of `scene`.

    For view r the points are those of `HipContext.depthmap_points`, all pixels, the map as it is
    (NaN depths are passed through, not replaced: such a pixel's point is NaN, sets no bit and is
    never kept); one rn_points_consistency call with exclude = r asks the other views.
    depthmap_points puts pixel (v, u) -- row v, column u -- at column u*H + v of its (3, H*W)
    table, the reference's order; THIS function is the one place where that order is undone: the
    four outputs come back as [W][H] and are transposed to (H, W)."""
    depth_maps = list(depth_maps)
    if scene is not None:
        if cameras is not None or frame_idxs is None:
            raise ValueError("a scene goes with frame_idxs and without cameras")
        cameras = [scene.get_image(int(i)).camera for i in frame_idxs]
    if cameras is None:
        raise ValueError("cameras, or a scene and frame_idxs, are required")
    cameras = list(cameras)
    _tolerances(tol_abs, tol_rel, border)
    V = len(cameras)
    if P_pinvs is None:
        P_pinvs = [c.P_pinv for c in cameras]
    if centers is None:
        centers = [c.center for c in cameras]
    if len(P_pinvs) != V or len(centers) != V:
        raise ValueError("%d cameras, %d P_pinvs and %d centers" % (V, len(P_pinvs), len(centers)))
    ctx = _context("checks depth maps")
    dev = ctx.device
    rows, depths = _views(cameras, depth_maps, dev)
    _, H, W = (int(s) for s in depths.shape)
    points = torch.empty((3, H * W), dtype=torch.float64, device=dev)
    results = []
    for r in range(V):
        pinv = torch.from_numpy(np.ascontiguousarray(P_pinvs[r], np.float64).reshape(4, 3)).to(dev)
        center = torch.from_numpy(np.ascontiguousarray(centers[r], np.float64).reshape(4)).to(dev)
        ctx.depthmap_points(H, W, pinv, center, depths[r], points)
        outs = ctx.points_consistency(points, rows, depths, r, tol_abs, tol_rel, border)
        # column u*H + v -> (H, W): the table is [W][H]
        seen, agree, violate, residual = (o.reshape(W, H).t().contiguous().cpu().numpy()
                                          for o in outs)
        own = depths[r].cpu().numpy()
        with np.errstate(invalid="ignore"):
            measured = (own > 0) & (own < np.inf)
        results.append(DepthConsistency(seen.view(np.uint32), agree.view(np.uint32),
                                        violate.view(np.uint32), residual, measured))
    return results
