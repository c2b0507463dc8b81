"""Depth maps -> point clouds on MI355X: the counterpart of raynet/pointcloud.py.

Same classes, constructor arguments and conventions as the reference (points are (3, N)
arrays, depth maps are the (H, W) float32 files / arrays the forward pass produces,
`scripts/forward_pass.py:136-142`); the work runs in HIP kernels (csrc/raynet_eval.inl):
back-projection and the multi-view consistency check in float64 like the NumPy code, the
nearest-neighbour queries as an exact brute-force scan instead of a host KD-tree.
"""
import sys

import numpy as np
import torch

from .hip_implementations import get_context


def _dev(x, dtype):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to("cuda", dtype).contiguous()


def _xyzw(points):
    """(3, N) -> [N][4] float32 device tensor."""
    p = _dev(points, torch.float32)
    out = torch.zeros((p.shape[1], 4), dtype=torch.float32, device="cuda")
    out[:, :3] = p.t()
    return out


class Pointcloud(object):
    """raynet/pointcloud.py:14-72."""

    def __init__(self, points):
        self._points = points

    @property
    def points(self):
        return self._points

    def save_ply(self, file):
        N = self.points.shape[1]
        with open(file, "wb") as f:
            f.write(("ply\nformat binary_%s_endian 1.0\ncomment Raynet pointcloud!\n"
                     "element vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                     "end_header\n" % (sys.byteorder, N)).encode())
            np.asarray(self.points).T.astype(np.float32).tofile(f)

    def save_colored_ply(self, file, intensities, colormap="jet"):
        """raynet/pointcloud.py:32-57: xyz float32 then uchar RGB per vertex, the colour of
        matplotlib's `colormap` at intensity / 2 (one value per point)."""
        from matplotlib import colormaps
        N = self.points.shape[1]
        values = np.asarray(intensities, np.float64).ravel() / 2
        if values.shape[0] != N:
            raise ValueError("%d intensities for %d points" % (values.shape[0], N))
        colors = (colormaps[colormap](values)[:, :-1] * 255).astype(np.uint8)
        vertices = np.empty((N,), dtype=[("xyz", np.float32, 3), ("rgb", np.uint8, 3)])
        vertices["xyz"] = np.asarray(self.points).T
        vertices["rgb"] = colors
        with open(file, "wb") as f:
            f.write(("ply\nformat binary_%s_endian 1.0\ncomment Raynet pointcloud!\n"
                     "element vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                     "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                     "end_header\n" % (sys.byteorder, N)).encode())
            vertices.tofile(f)

    def save_rgb_ply(self, file, colors):
        """xyz float32 then uchar RGB per vertex, the header layout of `save_colored_ply`;
        colors: (N, 3) uint8, e.g. what `colorize` returns."""
        N = self.points.shape[1]
        colors = np.asarray(colors)
        if colors.shape != (N, 3) or colors.dtype != np.uint8:
            raise ValueError("colors: expected uint8 of shape (%d, 3), got %s of shape %s"
                             % (N, colors.dtype, colors.shape))
        vertices = np.empty((N,), dtype=[("xyz", np.float32, 3), ("rgb", np.uint8, 3)])
        vertices["xyz"] = np.asarray(self.points).T
        vertices["rgb"] = colors
        with open(file, "wb") as f:
            f.write(("ply\nformat binary_%s_endian 1.0\ncomment Raynet pointcloud!\n"
                     "element vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                     "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                     "end_header\n" % (sys.byteorder, N)).encode())
            vertices.tofile(f)

    def colorize(self, scene, frame_idxs, depthmaps, tol, border=0, mode="blend",
                 unseen=(0.5, 0.5, 0.5)):
        """Colours of the points from the images of the scene's frames `frame_idxs` -> (colors
        (N, 3) uint8, views [N] uint32, bit k: frame_idxs[k] saw the point).  depthmaps: one per
        frame (.npy file names or arrays), the occluders: a frame sees a point that projects at
        least `border` pixels inside its image and is no farther from its camera than the map's
        value there plus `tol` (scene units).  There are no normals: every frame that sees a point
        weighs the same.  A point no frame sees gets `unseen`.  (appearance.project_colors)"""
        from .appearance import project_colors, scene_views, to_rgb8
        cameras, images = scene_views(scene, frame_idxs)
        if len(depthmaps) != len(cameras):
            raise ValueError("%d depth maps for %d frames" % (len(depthmaps), len(cameras)))
        maps = [np.load(d) if isinstance(d, str) else d for d in depthmaps]
        got = project_colors(np.ascontiguousarray(np.asarray(self.points).T, dtype=np.float32),
                             cameras, images, maps, None, tol=tol, border=border, mode=mode)
        return to_rgb8(got.colors, got.seen, unseen), got.views

    def save(self, file):
        np.save(file, self.points)

    def filter(self, mask):
        self._points = mask.filter(self.points)

    def index(self, leaf_size=40, metric="minkowski"):
        """The reference builds a KD-tree here; the scan needs no index, only the points on
        the device (kept until the cloud changes)."""
        pts = self.points
        if getattr(self, "_index", None) is None or self._index[0] is not pts:
            self._index = (pts, _xyzw(pts))

    def nearest_neighbors(self, X, k=1, return_distances=True):
        """Like KDTree.query(X.T, 1): ((Nq, 1) distances, (Nq, 1) indices) of the closest
        point of this cloud for every column of X."""
        assert k == 1, "only the nearest neighbour (what the metrics use) is implemented"
        self.index()
        ctx = get_context()
        q = _xyzw(X)
        dist = torch.empty((q.shape[0],), dtype=torch.float32, device="cuda")
        idx = torch.empty((q.shape[0],), dtype=torch.int32, device="cuda")
        ctx.nearest_neighbors(self._index[1], q, dist, idx)
        idx = idx.cpu().numpy().astype(np.int64).reshape(-1, 1)
        if not return_distances:
            return idx
        return dist.cpu().numpy().astype(np.float64).reshape(-1, 1), idx


class PointcloudFromDepthMaps(Pointcloud):
    """raynet/pointcloud.py:76-160.  depthmaps: .npy file names (as the reference) or arrays.
    confidences (file names or arrays like depthmaps, one per frame: the forward pass's
    `confidence` maps) and min_confidence: pixels whose confidence is below the threshold are
    dropped with the unwanted ones; keep_masks (one (H, W) bool array per frame, e.g.
    consistency.DepthConsistency.keep()): pixels that are False there are dropped too; the
    defaults select what the reference selects."""

    def __init__(self, scene, frame_idxs, depthmaps, borders=40, confidences=None,
                 min_confidence=0.0, keep_masks=None):
        self._scene = scene
        self._frame_idxs = frame_idxs
        self._depthmaps = depthmaps
        self._borders = borders
        self._points = None
        self._min_confidence = float(min_confidence)
        if confidences is not None and len(confidences) != len(frame_idxs):
            raise ValueError("%d confidence maps for %d frames" % (len(confidences), len(frame_idxs)))
        if confidences is None and self._min_confidence > 0:
            raise ValueError("min_confidence=%g needs the confidence maps" % self._min_confidence)
        self._confidence_of = dict(zip(frame_idxs, confidences)) if confidences is not None else None
        if keep_masks is not None and len(keep_masks) != len(frame_idxs):
            raise ValueError("%d keep masks for %d frames" % (len(keep_masks), len(frame_idxs)))
        self._keep_of = dict(zip(frame_idxs, keep_masks)) if keep_masks is not None else None

    @staticmethod
    def _load(d):
        return np.load(d) if isinstance(d, str) else np.asarray(d)

    def _selected_pixels(self, G, confidence=None, keep_mask=None):
        """Indices u*H + v of the pixels that survive _remove_unwanted_points
        (pointcloud.py:91-119), in the reference's order -- and, given the frame's confidence
        map, whose confidence is not below min_confidence, and, given the frame's keep mask,
        which are True there."""
        H, W = G.shape
        b = self._borders
        idxs = torch.arange(H * W, device="cuda").reshape(W, H).t()
        G = _dev(G, torch.float32)
        sl = (slice(b, H - b), slice(b, W - b))
        keep = G[sl] != 0
        if confidence is not None:
            C = _dev(self._load(confidence), torch.float32)
            if tuple(C.shape) != (H, W):
                raise ValueError("confidence map %s for a %s depth map" % (tuple(C.shape), (H, W)))
            keep = keep & ~(C[sl] < self._min_confidence)
        if keep_mask is not None:
            K = _dev(np.asarray(keep_mask), torch.bool)
            if tuple(K.shape) != (H, W):
                raise ValueError("keep mask %s for a %s depth map" % (tuple(K.shape), (H, W)))
            keep = keep & K[sl]
        return idxs[sl][keep]

    def _all_points(self, frame, depth):
        """(3, H*W) float64 device points of every pixel of `frame` (pointcloud.py:121-147)."""
        ctx = get_context()
        cam = self._scene.get_image(frame).camera
        depth = _dev(depth, torch.float32)
        bad = torch.isnan(depth)
        if bool(bad.any()):
            depth = torch.where(bad, depth[~bad].min(), depth)      # pointcloud.py:127
        H, W = depth.shape
        pts = torch.empty((3, H * W), dtype=torch.float64, device="cuda")
        ctx.depthmap_points(H, W, _dev(cam.P_pinv, torch.float64),
                            _dev(np.asarray(cam.center).reshape(4), torch.float64), depth, pts)
        return pts

    def _generate_points_per_image(self, frame, predicted_depth):
        depth = self._load(predicted_depth)
        sel = self._selected_pixels(
            self._scene.get_depth_map(frame),
            self._confidence_of[frame] if self._confidence_of is not None else None,
            self._keep_of[frame] if self._keep_of is not None else None)
        return self._all_points(frame, depth)[:, sel]

    @property
    def points(self):
        if self._points is None:
            pts = [self._generate_points_per_image(i, d)
                   for i, d in zip(self._frame_idxs, self._depthmaps)]
            self._points = torch.cat(pts, dim=1).cpu().numpy()
        return self._points


class PointcloudFromDepthMapsWithConsistency(PointcloudFromDepthMaps):
    """raynet/pointcloud.py:162-246."""

    def __init__(self, scene, frame_idxs, depthmaps, borders=40, consistency_threshold=0.75,
                 n_neighbors=5, confidences=None, min_confidence=0.0):
        self._consistency_threshold = consistency_threshold
        self._n_neighbors = n_neighbors
        self._camera_neighbors = None
        self._frame_idxs_map = dict(zip(frame_idxs, range(len(frame_idxs))))
        super(PointcloudFromDepthMapsWithConsistency, self).__init__(
            scene, frame_idxs, depthmaps, borders, confidences, min_confidence)

    def _neighbor_frames(self, frame):
        if self._camera_neighbors is None:
            a = np.hstack([np.asarray(self._scene.get_image(i).camera.center,
                                      np.float64).reshape(4, 1) for i in self._frame_idxs])
            distances = 2 * (a * a).sum(axis=0) - 2 * (a.T.dot(a))
            self._camera_neighbors = distances.argsort()[:, 1:self._n_neighbors + 1]
        return [(self._frame_idxs[i], self._depthmaps[i])
                for i in self._camera_neighbors[self._frame_idxs_map[frame]]]

    def _generate_points_per_image(self, frame, predicted_depth):
        ctx = get_context()
        pts = super(PointcloudFromDepthMapsWithConsistency, self)._generate_points_per_image(
            frame, predicted_depth).contiguous()
        tau = torch.empty((pts.shape[1],), dtype=torch.float64, device="cuda")
        for k, (i, d) in enumerate(self._neighbor_frames(frame)):
            cam = self._scene.get_image(i).camera
            depth = _dev(self._load(d), torch.float32)      # raw map, NaNs included (:232)
            H, W = depth.shape
            ctx.consistency_tau(H, W, k == 0, pts, _dev(cam.P, torch.float64),
                                _dev(np.asarray(cam.center).reshape(4), torch.float64), depth, tau)
        return pts[:, tau < self._consistency_threshold]


def get_pointcloud(scene, frame_idxs, depthmaps, with_consistency, **kwargs):
    """raynet/pointcloud.py:248-269; optional kwargs confidences, min_confidence and, without the
    reference's consistency check, keep_masks."""
    conf = dict(confidences=kwargs.get("confidences"),
                min_confidence=kwargs.get("min_confidence", 0.0))
    if kwargs.get("keep_masks") is not None:
        if with_consistency:
            raise ValueError("keep_masks and the reference's consistency check exclude each other")
        conf["keep_masks"] = kwargs["keep_masks"]
    if with_consistency:
        return PointcloudFromDepthMapsWithConsistency(
            scene, frame_idxs, depthmaps, kwargs["borders"], kwargs["consistency_threshold"],
            kwargs["n_neighbors"], **conf)
    return PointcloudFromDepthMaps(scene, frame_idxs, depthmaps, kwargs["borders"], **conf)
