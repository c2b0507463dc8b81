"""Depth maps fused into a truncated signed distance volume, restated in NumPy (DESIGN.md section
21, include/raynet_hip.h: rn_tsdf_integrate): the definition the GPU tests hold the kernel to bit
for bit, the cleaning of the mesh taken from the volume, and an analytic scene.

Everything is np.float64 arithmetic, one ufunc per operation and in the definition's order (NumPy
fuses nothing), vectorised over the voxels with a Python loop over the views.  Nothing here is
taken from the kernel.
"""
import numpy as np

# (the camera rows [V, 15] float64, P row-major | centre, the camera that looks straight down, and
# the projection of points by one row)
from appearance_truth import PlaneCamera, pack_cameras, project_points  # noqa: F401

F = np.float32
D = np.float64


def axes_of(bbox, grid_shape):
    """The three float32 tables of voxel centres of a grid, as the package lays them out."""
    from raynet_amd.common.scene import get_voxel_grid
    vg = get_voxel_grid(bbox, grid_shape)
    return [vg[0, :, 0, 0], vg[1, 0, :, 0], vg[2, 0, 0, :]]


def integrate(axes, cameras, depths, weights, trunc, border, order=None, sums=False):
    """axes: three float32 tables of voxel centres; cameras [V, 15] f64; depths [V, H, W] f32;
    weights [V, H, W] f32 or None -> (tsdf [gx, gy, gz] f32, weight [gx, gy, gz] f32).  order: the
    sequence the views are visited in (default: ascending, the definition's); sums: the float64
    (num, den) [G] instead."""
    ax = [np.asarray(a, F).astype(D) for a in axes]
    shape = tuple(len(a) for a in ax)
    x, y, z = [g.reshape(-1) for g in np.meshgrid(*ax, indexing="ij")]
    cameras = np.asarray(cameras, D).reshape(-1, 15)
    depths = np.asarray(depths, F)
    V, H, W = depths.shape
    assert len(cameras) == V
    if weights is not None:
        weights = np.asarray(weights, F)
        assert weights.shape == depths.shape
    trunc, border = D(trunc), D(border)
    G = len(x)
    num, den = np.zeros(G, D), np.zeros(G, D)
    with np.errstate(all="ignore"):
        x_max, y_max = D(W - 1) - border, D(H - 1) - border
        for v in (range(V) if order is None else order):
            X, Y, _, _, _, dd, ok = project_points(cameras[v], x, y, z, border, x_max, y_max)
            # a view that does not count reads pixel (0, 0)
            xi = np.rint(np.where(ok, X, 0.0)).astype(np.int64)
            yi = np.rint(np.where(ok, Y, 0.0)).astype(np.int64)
            zm = depths[v][yi, xi].astype(D)
            ok = ok & (zm > 0) & (zm < np.inf)
            if weights is not None:
                w = weights[v][yi, xi].astype(D)
                ok = ok & (w > 0) & (w < np.inf)
            else:
                w = np.ones(G, D)
            s = (zm * zm - dd) / (zm + zm)
            ok = ok & (s >= -trunc)
            t = np.minimum(s / trunc, 1.0)
            num = np.where(ok, num + w * t, num)
            den = np.where(ok, den + w, den)
        if sums:
            return num, den
        seen = den > 0
        tsdf = np.where(seen, (num / den).astype(F), F(1.0)).astype(F)
        weight = np.where(seen, den.astype(F), F(0.0)).astype(F)
    return tsdf.reshape(shape), weight.reshape(shape)


def field(tsdf, weight, min_weight=0.0):
    """The field whose zero level is the surface: -tsdf where the voxel was observed (weight > 0
    and weight >= min_weight), NaN elsewhere."""
    tsdf, weight = np.asarray(tsdf, F), np.asarray(weight, F)
    return np.where((weight > 0) & (weight >= F(min_weight)), -tsdf, F(np.nan)).astype(F)


def clean(vertices, faces):
    """Drops every face with a vertex that has a non-finite component, then every vertex no
    remaining face names, and renumbers; the order of both is kept."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    finite = np.isfinite(vertices).all(1)
    faces = faces[finite[faces].all(1)] if len(faces) else faces
    used = np.zeros(len(vertices), bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    return np.ascontiguousarray(vertices[used]), \
        np.ascontiguousarray(new[faces].astype(np.int32)).reshape(-1, 3)


def mesh(tsdf, weight, axes, bbox, min_weight=0.0, cleaned=True):
    """The mesh of a fused volume by the iso-surface's own restatement."""
    import isosurface_truth as it
    got = it.extract(field(tsdf, weight, min_weight), 0.0, False, axes, bbox)
    return clean(*got) if cleaned else got


# ------------------------------------------------------------------------------- the inputs
def sphere_depth(camera, H, W, centre, R):
    """[H, W] float32: the distance from the camera centre to the sphere (centre, R) along the
    ray of every pixel centre (whole coordinates), +inf where the ray misses it.  float64, from
    K, R and t of the camera (common.camera.Camera)."""
    K, Rm = np.asarray(camera.K, D), np.asarray(camera.R, D)
    c = np.asarray(camera.center, D).reshape(-1)[:3]
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    pix = np.stack([X, Y, np.ones_like(X)], -1)
    d = pix @ np.linalg.inv(K).T @ Rm                   # R^T K^-1 pix, as rows
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    oc = c - np.asarray(centre, D)
    b = d @ oc
    disc = b * b - (oc @ oc - D(R) * D(R))
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where((disc >= 0) & (t > 0), t, np.inf).astype(F)


def sphere_scene(H=120, W=160, grid=(24, 22, 20), V=8):
    """The unit sphere at the origin in the box +-1.6, seen by V cameras on a ring of radius 4 at
    elevations of +-0.5 rad -> dict(cameras, rows, depths, bbox, grid, axes, trunc)."""
    from raynet_amd.common.camera import Camera
    cams = []
    for v in range(V):
        a = 2 * np.pi * v / V + 0.1
        e = 0.5 if v % 2 == 0 else -0.5
        cams.append(Camera.look_at([4 * np.cos(a) * np.cos(e), 4 * np.sin(a) * np.cos(e),
                                    4 * np.sin(e)], [0, 0, 0], 1.1 * max(H, W), H, W))
    bbox = np.array([-1.6, -1.6, -1.6, 1.6, 1.6, 1.6], F)
    depths = np.stack([sphere_depth(c, H, W, (0, 0, 0), 1.0) for c in cams])
    side = float(max(3.2 / g for g in grid))
    return dict(cameras=cams, rows=pack_cameras(cams), depths=depths, bbox=bbox, grid=grid,
                axes=axes_of(bbox, grid), trunc=3 * side, side=side)

