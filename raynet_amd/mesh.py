"""Ground truth from scene meshes: first ray / mesh intersections on the GPU.

The reference finds the ground-truth depth of a pixel by casting its ray through an octree of
the scene's mesh, one Python call per pixel (raynet/common/scene.py:187-201,
utils/oct_tree.py, utils/training_utils.py:194-220, utils/fast_utils.pyx:47-117).
`MeshRaycaster` builds a bounding volume hierarchy of the triangles once, on the GPU, and casts
whole batches of rays through it (include/raynet_hip.h, rn_mesh_*):

  * the intersection test is the reference's Moeller-Trumbore in fp32, operation for operation;
  * the winner is the hit with the smallest fp32 squared distance to the origin, the lower
    triangle index on equal distances; only hits with t >= 0 count, and all of them count;
  * a pixel's ray runs from the camera centre (fp32) to project(P_pinv, (u, v, 1)) formed in
    float64 from the fp32 P_pinv and rounded once to fp32 (`pixel_destinations`);
  * a depth is the float64 distance of the hit to the camera centre (geometry.distance).

`closest_points` measures to the SURFACE (the reference's metrics measure to the mesh's vertices,
metrics.py:155-236) and `sample_surface` draws area-weighted points of it, for
metrics.SurfaceAccuracy / SurfaceCompleteness.

There is no CPU route: without a GPU the constructor raises RaynetHipError.
"""
import time

import numpy as np
import torch

from . import _lib


def pixel_destinations(P_pinv, us, vs):
    """[n, 3] f32 points project(P_pinv, (u, v, 1)) of pixels (u = column, v = row): the
    4x3 product formed in float64 from the fp32 P_pinv, ((P[k,0] u + P[k,1] v) + P[k,2]),
    divided by its last coordinate and rounded once to fp32 -- what k_mesh_depthmap computes."""
    P = np.asarray(P_pinv, dtype=np.float32).astype(np.float64).reshape(4, 3)
    u = np.asarray(us, dtype=np.float64).reshape(-1)
    v = np.asarray(vs, dtype=np.float64).reshape(-1)
    r = [(P[k, 0] * u + P[k, 1] * v) + P[k, 2] for k in range(4)]
    return np.stack([r[k] / r[3] for k in range(3)], axis=1).astype(np.float32)


def camera_origin(camera):
    """The camera centre as the rays' fp32 origin [3]."""
    return np.asarray(camera.center, dtype=np.float32).reshape(-1)[:3].copy()


def hit_depths(points, hit, center):
    """float64 distances of fp32 hit points [n, 3] to `center` (geometry.distance), NaN where
    `hit` is False."""
    c = np.asarray(center, dtype=np.float32).reshape(-1)[:3].astype(np.float64)
    d = np.asarray(points, dtype=np.float32).astype(np.float64) - c
    out = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    out[~np.asarray(hit, dtype=bool)] = np.nan
    return out


class MeshRaycaster(object):
    """BVH of a triangle soup [T, 9] (rows p0 | p1 | p2, float32), built once on the GPU.

    Attributes: `nodes` [max(T-1, 1), 16] f32 and `leaves` [T, 12] f32 (device tensors, layout
    in DESIGN.md section 14), `depth` (edges from the root to the deepest leaf) and
    `build_ms` (wall time of the build, synchronised)."""

    def __init__(self, triangles, device=None):
        if not torch.cuda.is_available():
            raise _lib.RaynetHipError(
                "no GPU visible: raynet_amd casts rays on MI355X only (no CPU fallback)")
        from .hip_implementations import get_context
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else int(device))
        if isinstance(triangles, torch.Tensor):
            tri = triangles.detach().to(device=self.device, dtype=torch.float32)
        else:
            tri = torch.from_numpy(np.ascontiguousarray(triangles, dtype=np.float32)).to(self.device)
        if tri.dim() != 2 or tri.shape[1] != 9 or tri.shape[0] < 1:
            raise ValueError("triangles: expected a non-empty [T, 9] array, got %s"
                             % (tuple(tri.shape),))
        if tri.shape[0] > (1 << 30):
            raise ValueError("triangles: at most 2^30 triangles")
        self.triangles = tri.contiguous()
        self.n_triangles = n = int(tri.shape[0])
        with torch.cuda.device(self.device):
            self._ctx = get_context()
            t0 = time.perf_counter()
            v = self.triangles.view(-1, 3)
            box = torch.cat([v.amin(0), v.amax(0)]).contiguous()
            keys = torch.empty((n,), dtype=torch.int64, device=self.device)
            self._ctx.mesh_keys(self.triangles, box, keys)
            keys = torch.sort(keys).values.contiguous()       # unique keys: a fixed order
            self.nodes = torch.empty((max(n - 1, 1), 16), dtype=torch.float32, device=self.device)
            self.leaves = torch.empty((n, 12), dtype=torch.float32, device=self.device)
            work = torch.empty((56 * n + 64,), dtype=torch.uint8, device=self.device)
            self.depth = self._ctx.mesh_build(self.triangles, keys, self.nodes, self.leaves, work)
            self.build_ms = (time.perf_counter() - t0) * 1e3
        self._area_cdf = None

    def first_intersections(self, origins, destinations):
        """First hits of the rays origins[i] -> destinations[i] ([n, 3] f32, host or device):
        (points [n, 3] f32, triangle [n] int32, -1 on a miss) as device tensors; a missed
        ray's point is (0, 0, 0)."""
        o = self._dev3(origins, "origins")
        d = self._dev3(destinations, "destinations")
        if o.shape != d.shape:
            raise ValueError("origins %s and destinations %s differ in shape"
                             % (tuple(o.shape), tuple(d.shape)))
        n = o.shape[0]
        points = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        tri = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._ctx.mesh_raycast(o, d, self.nodes, self.leaves, points, tri)
        return points, tri

    def depth_map(self, camera, H, W):
        """[H, W] f32 device tensor: every pixel's distance to the camera centre along its
        ray, 0 where the ray hits nothing ("0 = unknown", metrics.py)."""
        P = torch.from_numpy(np.asarray(camera.P_pinv, dtype=np.float32).reshape(12).copy())
        c = torch.from_numpy(camera_origin(camera))
        out = torch.empty((int(H), int(W)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            self._ctx.mesh_depthmap(H, W, P.to(self.device), c.to(self.device), self.nodes,
                                    self.leaves, out)
        return out

    def depth_for_pixels(self, camera, ys, xs):
        """float64 depths [n] of pixels (row ys[k], column xs[k]), NaN where the ray misses."""
        dst = pixel_destinations(camera.P_pinv, xs, ys)
        o = np.repeat(camera_origin(camera)[None], len(dst), axis=0)
        points, tri = self.first_intersections(o, dst)
        tri = tri.cpu().numpy()
        return hit_depths(points.cpu().numpy(), tri >= 0, camera.center)

    def closest_points(self, points):
        """The nearest point of the surface for every row of `points` ([n, 3], host or device,
        any float dtype; taken as float64): device tensors (dist f64 [n], closest f64 [n, 3],
        tri int32 [n]).  The surface is the leaves' triangles p0, p0 + e1, p0 + e2 in float64
        -- the triangles the rays hit; a zero-area triangle is the segment or point it is."""
        if isinstance(points, torch.Tensor):
            q = points.detach().to(device=self.device, dtype=torch.float64)
        else:
            q = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).to(self.device)
        if q.dim() != 2 or q.shape[1] != 3:
            raise ValueError("points: expected [n, 3], got %s" % (tuple(q.shape),))
        q = q.contiguous()
        n = q.shape[0]
        dist = torch.empty((n,), dtype=torch.float64, device=self.device)
        closest = torch.empty((n, 3), dtype=torch.float64, device=self.device)
        tri = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._ctx.mesh_closest(q, self.nodes, self.leaves, dist, closest, tri)
        return dist, closest, tri

    @property
    def area_cdf(self):
        """Inclusive running sum [T] f64 (device) of the triangles' areas 0.5 |e1 x e2| in the
        caller's triangle order, taken once."""
        if self._area_cdf is None:
            with torch.cuda.device(self.device):
                areas = torch.empty((self.n_triangles,), dtype=torch.float64, device=self.device)
                self._ctx.mesh_areas(self.triangles, areas)
                self._area_cdf = torch.cumsum(areas, 0).contiguous()
        return self._area_cdf

    @property
    def area(self):
        """The surface's area (a Python float): the last entry of `area_cdf`."""
        return float(self.area_cdf[-1].item())

    def sample_surface(self, n_samples, seed=0):
        """`n_samples` stratified, area-weighted points of the surface: (points f32 [n, 3],
        tri int32 [n]) as device tensors, the same for the same mesh, n_samples and seed.
        Sample k lies in the first triangle t with area_cdf[t] > (k + r0) / n * area (so never in
        a zero-area one) at p0 + r1 e1 + r2 e2; the hash behind r0, r1, r2: DESIGN.md section 14."""
        n = int(n_samples)
        if n < 0 or n > (1 << 30):
            raise ValueError("n_samples: 0 .. 2^30, got %d" % n)
        seed = int(seed)
        if not -(1 << 63) <= seed < (1 << 63):
            raise ValueError("seed: a signed 64-bit integer")
        if n and not self.area > 0.0:
            raise ValueError("the mesh has no area to sample (%r)" % self.area)
        points = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        tri = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._ctx.mesh_sample(self.triangles, self.area_cdf, seed, points, tri)
        return points, tri

    def _dev3(self, x, name):
        if isinstance(x, torch.Tensor):
            t = x.detach().to(device=self.device, dtype=torch.float32)
        else:
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("%s: expected [n, 3], got %s" % (name, tuple(t.shape)))
        return t.contiguous()
