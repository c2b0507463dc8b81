"""Which views to use: the views that see each point of a proxy geometry, the points every pair of
views shares at a useful triangulation angle, a view's best neighbours and a greedy covering set
(DESIGN.md section 30).

The work is two HIP kernels (csrc/raynet_overlap.inl; the definitions are in include/raynet_hip.h
at rn_view_overlap / rn_view_gain).  A view sees a point by rn_project_colors's tests -- it
projects into the image, faces the view, is not behind the view's depth map -- and two views share
a point both see when the angle between its rays to their centres lies in [min_angle, max_angle].
Here is the plumbing: the cameras packed as rows of 15 float64, the degrees turned into cosines (so
that no libm call enters the kernel), the pair matrix mirrored, and the orderings: `neighbors`
sorts a row of the matrix, `cover` runs the greedy loop with one rn_view_gain launch per pick.

Up to 64 views per call.  There is no CPU route: without a GPU the functions raise RaynetHipError.
"""
import numpy as np
import torch

from .appearance import _context, _dev, pack_cameras

MAX_VIEWS = 64


def band_cosines(min_angle, max_angle):
    """(cos_lo, cos_hi) of a band of triangulation angles in degrees, 0 <= min_angle <= max_angle
    <= 90: the cosines of the largest and of the smallest angle, 0 and 1 exactly at 90 and 0."""
    if not (0.0 <= min_angle <= max_angle <= 90.0):
        raise ValueError("min_angle, max_angle: degrees with 0 <= min_angle <= max_angle <= 90, "
                         "got %r, %r" % (min_angle, max_angle))
    cos_lo = 0.0 if max_angle == 90.0 else float(np.cos(np.deg2rad(np.float64(max_angle))))
    cos_hi = 1.0 if min_angle == 0.0 else float(np.cos(np.deg2rad(np.float64(min_angle))))
    return min(max(cos_lo, 0.0), 1.0), min(max(cos_hi, 0.0), 1.0)


class ViewOverlap(object):
    """What `view_overlap` returns: visible [n] uint64 (bit v: view v sees point p) and pairs
    (V, V) int64, symmetric -- pairs[i, i] the number of points view i sees, pairs[i, j] the
    number of points views i and j share -- as host arrays; the masks stay on the device for
    `cover`."""

    def __init__(self, visible, pairs, device_visible=None, context=None):
        self.visible = np.ascontiguousarray(visible, np.uint64)
        self.pairs = np.ascontiguousarray(pairs, np.int64)
        self.n_views = len(self.pairs)
        if self.pairs.shape != (self.n_views, self.n_views) or not 1 <= self.n_views <= MAX_VIEWS:
            raise ValueError("pairs: a (V, V) matrix of 1 to %d views, got %s"
                             % (MAX_VIEWS, self.pairs.shape))
        self._device_visible, self._context = device_visible, context

    def neighbors(self, i, k):
        """The k views j != i with the largest pairs[i, j]: ties go to the lower j, and views that
        share nothing with i come last, in index order."""
        i, k = int(i), int(k)
        if not 0 <= i < self.n_views:
            raise ValueError("i: a view 0..%d, got %d" % (self.n_views - 1, i))
        if k < 0:
            raise ValueError("k: 0 or more, got %d" % k)
        row = sorted((-int(self.pairs[i, j]), j) for j in range(self.n_views) if j != i)
        return [j for _, j in row][:k]

    def _gain(self, chosen, redundancy):
        """[V + 1] Python ints: one rn_view_gain launch on a zeroed gain."""
        if self._device_visible is None:
            ctx = _context("chooses views")
            self._context = ctx
            self._device_visible = torch.from_numpy(self.visible.view(np.int64)).to(ctx.device)
        gain = self._context.view_gain(self._device_visible, self.n_views, chosen, redundancy)
        return [int(g) for g in gain.cpu().numpy()]

    def cover(self, k, redundancy=1, candidates=None):
        """A greedy covering set of at most k views -> (order, gains, short).  A point is short
        while fewer than `redundancy` chosen views see it; every round takes the view (of
        `candidates`, default all) that sees the most short points, ties going to the lower index,
        and the loop stops at k views or when no view sees a short point.  order: the views in
        the order chosen; gains: the short points each saw when chosen; short: the points still
        short at the end."""
        k, redundancy = int(k), int(redundancy)
        if k < 0:
            raise ValueError("k: 0 or more, got %d" % k)
        if not 1 <= redundancy <= MAX_VIEWS:
            raise ValueError("redundancy: 1 to %d, got %d" % (MAX_VIEWS, redundancy))
        allowed = list(range(self.n_views)) if candidates is None else \
            sorted(set(int(c) for c in candidates))
        if allowed and not 0 <= allowed[0] <= allowed[-1] < self.n_views:
            raise ValueError("candidates: views 0..%d, got %r" % (self.n_views - 1, candidates))
        chosen, order, gains = 0, [], []
        gain = self._gain(chosen, redundancy)
        while len(order) < k:
            best, best_gain = -1, 0
            for v in allowed:
                if not (chosen >> v) & 1 and gain[v] > best_gain:
                    best, best_gain = v, gain[v]
            if best < 0:
                break
            order.append(best)
            gains.append(best_gain)
            chosen |= 1 << best
            gain = self._gain(chosen, redundancy)
        return order, gains, gain[self.n_views]


def _scalars(tol, min_cos, border):
    for name, value in (("tol", tol), ("min_cos", min_cos), ("border", border)):
        if not (value >= 0.0 and np.isfinite(value)):
            raise ValueError("%s: a finite number that is 0 or more, got %r" % (name, value))


def view_overlap(points, cameras, image_shape, normals=None, depth_maps=None, tol=0.0, min_cos=0.0,
                 border=0.0, min_angle=2.0, max_angle=45.0):
    """Which of `cameras` see each of `points` (n, 3), and how many points every pair of cameras
    shares -> ViewOverlap.

    cameras: common.camera.Camera objects (P, center), at most 64; image_shape (H, W) of their
    images.  normals (n, 3): a view sees only points that face it (cos > min_cos); a zero normal
    faces everything.  depth_maps: one (H, W) map per camera of distances to the camera centre,
    the occluders -- a view sees a point no farther than its map's value at the point's pixel plus
    `tol` (scene units); None: nothing occludes.  border: pixels to stay away from the image's
    edge.  Two views share a point both see when the angle between the point's rays to the two
    centres lies in [min_angle, max_angle] degrees."""
    cameras = list(cameras)
    V = len(cameras)
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError("%d views: 1 to %d per call (a bit of the mask each)" % (V, MAX_VIEWS))
    _scalars(tol, min_cos, border)
    cos_lo, cos_hi = band_cosines(min_angle, max_angle)
    H, W = (int(s) for s in image_shape)
    if H < 1 or W < 1:
        raise ValueError("image_shape: (H, W) of 1 or more, got %r" % (image_shape,))
    p = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points: expected shape (n, 3), got %s" % (p.shape,))
    nr = None
    if normals is not None:
        nr = np.asarray(normals.detach().cpu() if isinstance(normals, torch.Tensor) else normals)
        if nr.shape != p.shape:
            raise ValueError("normals: expected shape %s, got %s" % (p.shape, nr.shape))
    if depth_maps is not None:
        depth_maps = list(depth_maps)
        shapes = [tuple(np.shape(d)) for d in depth_maps]       # (device tensors stay where they are)
        if len(depth_maps) != V or any(s != (H, W) for s in shapes):
            raise ValueError("depth_maps: %d maps of %s, got %d of %s" % (
                V, (H, W), len(depth_maps), sorted(set(shapes))))
    ctx = _context("chooses views")
    dev = ctx.device
    pts = torch.from_numpy(np.ascontiguousarray(p.T, dtype=np.float64)).to(dev)
    nrm = None if nr is None else torch.from_numpy(np.ascontiguousarray(nr.T, dtype=np.float64)).to(dev)
    depths = None if depth_maps is None else \
        torch.stack([_dev(d, torch.float32, dev) for d in depth_maps])
    rows = torch.from_numpy(pack_cameras(cameras)).to(dev)
    visible, pairs = ctx.view_overlap(pts, nrm, rows, (H, W), depths, tol, min_cos, border, cos_lo,
                                      cos_hi)
    upper = pairs.cpu().numpy()
    return ViewOverlap(visible.cpu().numpy().view(np.uint64), np.triu(upper) + np.triu(upper, 1).T,
                       visible, ctx)
