"""Sampling schemes: WHERE on the viewing ray the D samples lie.

API mirror of raynet/common/sampling_schemes.py:10-297 -- `get_sampling_scheme(name)` and classes
with the reference's three methods and shapes -- with the points computed on the GPU by K8
(`rn_sample_points` / `rn_sample_points_scheme`, include/raynet_hip.h "sampling schemes"):

    sample_points_across_ray(scene, i, y, x)            (n_points, 4) float32, or None
    sample_points_across_rays(scene, i)                 (4, H * W, n_points) float32
    sample_points_across_rays_batched(scene, i, batch)  (4, len(batch), n_points) float32

Rays are enumerated as the reference does (u-major: ray = x * H + y).  A `sample_in_disparity`
ray that misses the box has no samples: the per-ray method returns None as the reference does,
the vectorised ones hand its D points out as the camera centre with w = 0 (every other point
has w = 1) -- `missed_rays(points)` reads that flag.  `sample_in_disparity`'s far view is the
last of `scene.get_image_with_neighbors(i, neighbors)`.
"""
import numpy as np

SCHEME_OF_SAMPLING_TYPE = {None: "sample_in_bbox", "sample_points_in_bbox": "sample_in_bbox",
                           "sample_points_in_range": "sample_in_range",
                           "sample_points_in_disparity": "sample_in_disparity"}


def scheme_name(generation_params):
    """The --sampling_policy name behind generation_params.sampling_type (which holds the
    routine's name, generation_parameters.py:20-28; None: the default, sample_in_bbox)."""
    st = getattr(generation_params, "sampling_type", None)
    if st in SCHEME_OF_SAMPLING_TYPE:
        return SCHEME_OF_SAMPLING_TYPE[st]
    if st in SCHEME_OF_SAMPLING_TYPE.values():
        return st
    raise NotImplementedError(st)


def far_view_of(images):
    """(P, P_pinv, centre) float32 of the last view of [reference, neighbours...]."""
    cam = images[-1].camera
    return (np.asarray(cam.P, np.float32), np.asarray(cam.P_pinv, np.float32),
            np.asarray(cam.center, np.float32).ravel())


def missed_rays(points):
    """Rays without samples in a (4, N, D) result: bool [N]."""
    return np.asarray(points)[3, :, 0] == 0


class SamplingScheme(object):
    name = None

    def __init__(self, generation_params):
        self.sampling_type = generation_params.sampling_type
        self.n_points = generation_params.depth_planes
        self._neighbors = getattr(generation_params, "neighbors", 4)
        self._range = getattr(generation_params, "depth_range", None)

    def _sample(self, scene, i, ray_idxs):
        """(len(ray_idxs), n_points, 4) float32 from K8."""
        import torch

        from ..hip_implementations.sample_points import batch_sample_points
        H, W = scene.image_shape
        kw = {}
        if self.name == "sample_in_range":
            kw["depth_range"] = self._range
        sp = batch_sample_points(self.n_points, H, W, np.asarray(scene.bbox, np.float32).ravel(),
                                 self.name, **kw)
        ctx = sp.context
        cam = scene.get_image(i).camera
        ridx = ctx.dev(np.ascontiguousarray(ray_idxs, dtype=np.int32))
        pts = torch.zeros((len(ridx), self.n_points, 4), dtype=torch.float32, device=ctx.device)
        kw = {}
        if self.name == "sample_in_disparity":
            kw["far_view"] = far_view_of(scene.get_image_with_neighbors(i, self._neighbors))
        sp(ridx, np.asarray(cam.P_pinv, np.float32), np.asarray(cam.center, np.float32).ravel(),
           pts, **kw)
        return pts.cpu().numpy()

    def sample_points_across_ray(self, scene, i, y, x):
        H, _ = scene.image_shape
        p = self._sample(scene, i, [int(x) * H + int(y)])[0]
        return None if p[0, 3] == 0 else p

    def sample_points_across_rays(self, scene, i):
        H, W = scene.image_shape
        return self._sample(scene, i, np.arange(H * W)).transpose(2, 0, 1)

    def sample_points_across_rays_batched(self, scene, i, batch):
        H, W = scene.image_shape
        return self._sample(scene, i, np.arange(H * W)[batch]).transpose(2, 0, 1)


class SamplingInBboxScheme(SamplingScheme):
    """sampling_schemes.py:99-175.  (The reference's per-ray method returns None for a ray that
    misses the box and its vectorised one samples it all the same; K8 samples it in both.)"""
    name = "sample_in_bbox"

    def sample_points_across_ray(self, scene, i, y, x):
        H, _ = scene.image_shape
        return self._sample(scene, i, [int(x) * H + int(y)])[0]


class SamplingInRangeScheme(SamplingScheme):
    """sampling_schemes.py:178-237: depth_range = generation_params.depth_range."""
    name = "sample_in_range"

    def __init__(self, generation_params):
        super(SamplingInRangeScheme, self).__init__(generation_params)
        if self._range is None:
            raise ValueError("sample_in_range needs generation_params.depth_range")


class SamplingInDisparityScheme(SamplingScheme):
    """sampling_schemes.py:240-297."""
    name = "sample_in_disparity"


_SCHEMES = {c.name: c for c in (SamplingInBboxScheme, SamplingInRangeScheme,
                                SamplingInDisparityScheme)}


def get_sampling_scheme(name):
    """sampling_schemes.py:417-426 for the schemes this package runs."""
    return _SCHEMES[name]
