"""Evaluation metrics of the reference (raynet/metrics.py:130-236) on MI355X: the same
classes and `compute(scene, frame_idxs, depthmaps, predicted_pointcloud)` signature; the
nearest-neighbour distances come from the HIP scan behind `Pointcloud.nearest_neighbors`.

`Accuracy` / `Completeness` measure to and from the ground-truth mesh's VERTICES, as the
reference does; on meshes of large flat triangles a point that lies exactly on a wall is then
far from the ground truth.  `SurfaceAccuracy` / `SurfaceCompleteness` measure to the mesh's
surface and from area-weighted samples of it (scene.get_surface(), raynet_amd/mesh.py).

`VoxelMask` / `ReduceDensity` are the reference's two filters (raynet/metrics.py:27-127) for a
`FiltersFactory`; the thinning runs as exact parallel rounds on the GPU (DESIGN.md section
12a) and, unlike the reference's unseeded shuffle, in a reproducible visiting order."""
import os
import time

import numpy as np

from .pointcloud import Pointcloud, PointcloudFromDepthMaps  # noqa: F401


class FiltersFactory(object):
    """raynet/metrics.py:11-24."""

    def __init__(self, filters):
        self.filters = filters

    @property
    def has_filters(self):
        return len(self.filters) > 0

    def filter(self, X):
        for f in self.filters:
            X = f.filter(X)
        return X


def _as_points(X):
    """(3, N) NumPy array or tensor -> (3, N) float64 NumPy array (float32 is widened)."""
    if hasattr(X, "detach"):
        X = X.detach().cpu().numpy()
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] != 3:
        raise ValueError("points must be (3, N), got %s" % (X.shape,))
    return np.ascontiguousarray(X, dtype=np.float64)


def _filtered(X, keep, output_directory, file_name):
    """The reference's tail of a filter: the kept columns in their original order, its
    message, and the PLY when an output directory is set."""
    points = np.ascontiguousarray(X[:, keep])
    print("Filter out %d out of %d points" % (X.shape[1] - points.shape[1], X.shape[1]))
    if output_directory is not None:
        Pointcloud(points).save_ply(os.path.join(output_directory, file_name))
    return points


class VoxelMask(object):
    """raynet/metrics.py:27-75: keep the points inside the closed bounding box whose voxel of
    `mask` is 1.  bbox: (1, 6); mask: (A, B, C).  One deviation: a point on the max face of an
    axis with an even voxel count indexes one past the mask in the reference (IndexError);
    here that index is clamped to the last voxel."""

    def __init__(self, bbox, mask, output_directory=None):
        bbox = np.asarray(bbox)
        mask = np.asarray(mask)
        if bbox.shape != (1, 6) or mask.ndim != 3:
            raise ValueError("bbox must be (1, 6) and mask (A, B, C)")
        if not np.all(bbox[0, :3] < bbox[0, 3:]):
            raise ValueError("bbox: min must be below max on every axis")
        self._bbox_min = bbox[0, :3, np.newaxis]
        self._bbox_max = bbox[0, 3:, np.newaxis]
        self._grid_shape = np.array(mask.shape).reshape(3, 1)
        self._mask = mask
        # NumPy's own promotion: the float32 difference over the int64 shape is float64
        self._steps = (self._bbox_max - self._bbox_min) / self._grid_shape
        self.output_directory = output_directory

    def _box(self):
        """min | max | step | step / 2 as the float64 values NumPy uses next to float64 points."""
        return np.concatenate([a.astype(np.float64).ravel() for a in (
            self._bbox_min, self._bbox_max, self._steps, self._steps / 2)])

    def filter(self, X):
        import torch
        from .hip_implementations import get_context
        X = _as_points(X)
        N = X.shape[1]
        if N == 0:
            return _filtered(X, np.zeros((0,), bool), self.output_directory,
                             "pc_inside_voxel_mask.ply")
        keep = torch.empty((N,), dtype=torch.uint8, device="cuda")
        get_context().voxel_mask(
            torch.from_numpy(X).cuda(), torch.from_numpy(self._box()).cuda(),
            torch.from_numpy(np.ascontiguousarray(self._mask == 1).view(np.uint8)).cuda(), keep)
        return _filtered(X, keep.cpu().numpy().astype(bool), self.output_directory,
                         "pc_inside_voxel_mask.ply")


_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix64(z):
    """splitmix64's output function on a uint64 array (modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def priority_hash(seed, n):
    """The visiting priorities k_thin_keys gives n points without an explicit order:
    mix64(mix64(seed + G) + G * (i + 1)), uint64 (include/raynet_hip.h: rn_thin_keys)."""
    key = _mix64(np.array([(int(seed) + _GOLDEN) & _MASK64], np.uint64))
    return _mix64(key + np.uint64(_GOLDEN) * np.arange(1, n + 1, dtype=np.uint64))


class ReduceDensity(object):
    """raynet/metrics.py:78-127: thin a cloud so that no two kept points are within `min_dist`
    (dx*dx + dy*dy + dz*dz <= min_dist*min_dist in float64): visiting the points in an order,
    a point is kept iff no earlier-visited kept point is that close.  The reference shuffles
    with NumPy's unseeded global generator; here the order is the hash of (seed, index) --
    ascending `priority_hash(seed, N)`, ties by index -- or `order`, a permutation of range(N)
    visited first to last, which reproduces any given order (the reference's included)."""

    CELL_BITS = 21
    MAX_CELL = (1 << 21) - 3          # largest cell index per axis: its +1 neighbour, +1, fits

    def __init__(self, min_dist, output_directory=None, seed=0, order=None):
        if not min_dist > 0:
            raise ValueError("min_dist must be positive, got %r" % (min_dist,))
        self._min_dist = float(min_dist)
        self.output_directory = output_directory
        self.seed = int(seed)
        self.order = None if order is None else np.asarray(order)
        self.rounds = None            # rounds the last filter() took ...
        self.round_seconds = None     # ... and each one's wall time, its count's read included

    def visiting_order(self, n):
        """The order in use for n points: indices, first visited first."""
        if self.order is not None:
            return self._checked_order(n)
        return np.argsort(priority_hash(self.seed, n), kind="stable")

    def _checked_order(self, n):
        order = self.order
        ok = order.ndim == 1 and order.shape[0] == n and order.dtype.kind in "iu"
        if ok and n:
            order = order.astype(np.int64)
            ok = order.min() >= 0 and order.max() < n and \
                bool(np.all(np.bincount(order, minlength=n) == 1))
        if not ok:
            raise ValueError("order must be a permutation of range(%d)" % n)
        return order.astype(np.int64)

    def _grid(self, X):
        """(lo, h) of the search grid; ValueError for what the keys cannot hold."""
        if not np.isfinite(X).all():
            raise ValueError("points have non-finite coordinates")
        h = self._min_dist * (1.0 + 2.0 ** -20)
        lo = X.min(axis=1)
        ratio = (X.max(axis=1) - lo) / h
        for axis in range(3):
            if not np.floor(ratio[axis]) <= self.MAX_CELL:
                raise ValueError(
                    "the cloud's extent over the cell size is %.6g on axis %d; the cell keys "
                    "hold %d bits per axis, so it must stay below %d: choose a larger min_dist "
                    "or cut the cloud first (VoxelMask)"
                    % (ratio[axis], axis, self.CELL_BITS, self.MAX_CELL + 1))
        return lo, h

    def keep_mask(self, points, lo, h, position=None):
        """The device part: points (3, N) float64 CUDA tensor, position None or the (N,) int64
        CUDA tensor of every point's place in the order -> (N,) bool CUDA tensor of the kept
        points.  Synchronises once per round (the count of undecided points)."""
        import torch
        from .hip_implementations import get_context
        ctx = get_context()
        N = points.shape[1]
        keys = torch.empty((N,), dtype=torch.int64, device="cuda")
        priority = torch.empty((N,), dtype=torch.int64, device="cuda")
        ctx.thin_keys(points, lo, h, self.seed, position, keys, priority)
        # cell order: neighbouring lanes hold neighbouring points
        keys, perm = torch.sort(keys)
        points = points[:, perm].contiguous()
        priority = priority[perm].contiguous()
        index = perm.to(torch.int32)
        state = torch.zeros((N,), dtype=torch.int32, device="cuda")
        undecided = torch.zeros((1,), dtype=torch.int32, device="cuda")
        r2 = self._min_dist * self._min_dist
        torch.cuda.current_stream().synchronize()     # round_seconds[0] is the round's alone
        work, rounds, seconds = None, 0, []
        while True:
            t0 = time.perf_counter()
            undecided.zero_()
            ctx.thin_round(work, keys, points, priority, index, r2, state, undecided)
            rounds += 1
            left = int(undecided.item())
            seconds.append(time.perf_counter() - t0)
            if left == 0:
                break
            if rounds > N:
                raise RuntimeError("the thinning did not settle in N rounds")
            if work is None:
                work = torch.nonzero(state == 0).view(-1).to(torch.int32)
            else:
                work = work[state[work.long()] == 0].contiguous()
        self.rounds, self.round_seconds = rounds, seconds
        keep = torch.empty((N,), dtype=torch.bool, device="cuda")
        keep[perm] = state == 1
        return keep

    def filter(self, X):
        import torch
        X = _as_points(X)
        N = X.shape[1]
        position = None
        if self.order is not None:
            order = self._checked_order(N)
            position = np.empty((N,), np.int64)
            position[order] = np.arange(N, dtype=np.int64)
        if N == 0:
            keep = np.zeros((0,), bool)
        else:
            lo, h = self._grid(X)
            keep = self.keep_mask(torch.from_numpy(X).cuda(), lo, h,
                                  None if position is None else torch.from_numpy(position).cuda())
            keep = keep.cpu().numpy()
        return _filtered(X, keep, self.output_directory, "pc_after_density_reduction.ply")


class Metric(object):
    def compute(self, scene, frame_idxs, depthmaps, predicted_pointcloud):
        raise NotImplementedError()


class PerPixelMeanDepthError(Metric):
    """raynet/metrics.py:135-152."""

    def __init__(self, borders=40):
        self.borders = borders

    def compute(self, scene, frame_idxs, depthmaps, predicted_pointcloud):
        """-> (mean |ground truth - prediction| per frame over the pixels that HAVE ground
        truth, None); a frame's border of `borders` pixels is left out."""
        H, W = scene.image_shape
        b = self.borders
        inner = (slice(b, H - b), slice(b, W - b))

        def frame_error(frame, prediction):
            truth = scene.get_depth_map(frame)[inner]
            if isinstance(prediction, str):
                prediction = np.load(prediction)
            known = truth != 0
            return np.abs(truth[known] - np.asarray(prediction)[inner][known]).mean()

        errors = [frame_error(f, d) for f, d in zip(frame_idxs, depthmaps)]
        return np.array(errors, dtype=np.float64).reshape(len(frame_idxs)), None


class _CloudMetric(Metric):
    def __init__(self, filter_factory=None, truncate=float("inf"), borders=40,
                 use_pc_from_depthmap=False):
        self.filter_factory = filter_factory if filter_factory is not None else FiltersFactory([])
        self.truncate = truncate
        self.borders = borders
        self.use_pc_from_depthmap = use_pc_from_depthmap

    def _clouds(self, scene, frame_idxs, predicted_pointcloud):
        if self.use_pc_from_depthmap:
            # ground-truth cloud from the ground-truth depth maps (metrics.py:170-181)
            gt = [scene.get_depthmap_file(i) for i in frame_idxs]
            ground_truth_pc = PointcloudFromDepthMaps(scene, frame_idxs, gt, self.borders)
        else:
            ground_truth_pc = scene.get_pointcloud()
        if self.filter_factory.has_filters:
            ground_truth_pc.filter(self.filter_factory)
            predicted_pointcloud.filter(self.filter_factory)
        return ground_truth_pc


class Accuracy(_CloudMetric):
    """raynet/metrics.py:155-195: distance of every predicted point to the ground truth."""

    def compute(self, scene, frame_idxs, depthmaps, predicted_pointcloud):
        ground_truth_pc = self._clouds(scene, frame_idxs, predicted_pointcloud)
        ground_truth_pc.index()
        distances, indexes = ground_truth_pc.nearest_neighbors(predicted_pointcloud.points)
        return np.minimum(distances, self.truncate), predicted_pointcloud.points


class Completeness(_CloudMetric):
    """raynet/metrics.py:198-236: distance of every ground-truth point to the prediction."""

    def compute(self, scene, frame_idxs, depthmaps, predicted_pointcloud):
        ground_truth_pc = self._clouds(scene, frame_idxs, predicted_pointcloud)
        predicted_pointcloud.index()
        distances, indexes = predicted_pointcloud.nearest_neighbors(ground_truth_pc.points)
        return np.minimum(distances, self.truncate), ground_truth_pc.points


class SurfaceAccuracy(Metric):
    """Distance of every predicted point to the ground-truth SURFACE
    (scene.get_surface().closest_points, float64): -> ((N, 1) distances, predicted points)
    like Accuracy.  A scene without a mesh raises NotImplementedError."""

    def __init__(self, filter_factory=None, truncate=float("inf")):
        self.filter_factory = filter_factory if filter_factory is not None else FiltersFactory([])
        self.truncate = truncate

    def compute(self, scene, frame_idxs, depthmaps, predicted_pointcloud):
        surface = scene.get_surface()
        if self.filter_factory.has_filters:
            predicted_pointcloud.filter(self.filter_factory)
        points = predicted_pointcloud.points
        dist, _, _ = surface.closest_points(np.asarray(points).T)
        distances = dist.cpu().numpy().reshape(-1, 1)
        return np.minimum(distances, self.truncate), points


class SurfaceCompleteness(Metric):
    """Distance of `n_samples` area-weighted samples of the ground-truth surface
    (scene.get_surface().sample_surface(n_samples, seed)) to the prediction: from the samples
    on, Completeness."""

    def __init__(self, n_samples, seed=0, filter_factory=None, truncate=float("inf")):
        self.n_samples = n_samples
        self.seed = seed
        self.filter_factory = filter_factory if filter_factory is not None else FiltersFactory([])
        self.truncate = truncate

    def compute(self, scene, frame_idxs, depthmaps, predicted_pointcloud):
        samples, _ = scene.get_surface().sample_surface(self.n_samples, self.seed)
        ground_truth_pc = Pointcloud(np.ascontiguousarray(samples.cpu().numpy().T))
        if self.filter_factory.has_filters:
            ground_truth_pc.filter(self.filter_factory)
            predicted_pointcloud.filter(self.filter_factory)
        predicted_pointcloud.index()
        distances, indexes = predicted_pointcloud.nearest_neighbors(ground_truth_pc.points)
        return np.minimum(distances, self.truncate), ground_truth_pc.points


def photometric_error(rendered, image, mask):
    """The image-space score of a rendered surface against a photograph:
    rendered and image (H, W) or (H, W, C) arrays of one shape in [0, 1], mask (H, W) the pixels
    the surface covers -> dict(coverage, mae, mse, psnr), in NumPy float64.  coverage: the share
    of pixels covered; mae and mse: the mean absolute and the mean squared difference over the
    covered pixels and all channels; psnr = 10 log10(1 / mse), inf at mse == 0.  Nothing covered:
    coverage 0, the other three nan."""
    a, b = np.asarray(rendered, np.float64), np.asarray(image, np.float64)
    covered = np.asarray(mask, bool)
    if a.shape != b.shape or a.ndim not in (2, 3) or covered.shape != a.shape[:2]:
        raise ValueError("rendered %s, image %s and mask %s: (H, W[, C]) twice and (H, W)"
                         % (a.shape, b.shape, covered.shape))
    n = int(covered.sum())
    coverage = n / float(covered.size) if covered.size else 0.0
    if n == 0:
        return dict(coverage=coverage, mae=float("nan"), mse=float("nan"), psnr=float("nan"))
    diff = a[covered] - b[covered]
    mse = float((diff * diff).mean())
    psnr = float("inf") if mse == 0.0 else float(10.0 * np.log10(1.0 / mse))
    return dict(coverage=coverage, mae=float(np.abs(diff).mean()), mse=mse, psnr=psnr)
