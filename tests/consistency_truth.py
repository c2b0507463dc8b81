"""What the other views say about a point, restated in NumPy (DESIGN.md section 29,
include/raynet_hip.h: rn_points_consistency): the definition the GPU tests hold the kernel to bit
for bit, the keep rule of the package's DepthConsistency, and the perturbed plane scene.

Everything is np.float64 arithmetic, one ufunc per operation and in the definition's order (NumPy
fuses nothing), vectorised over the points with a Python loop over the views.  Nothing here is
taken from the kernel.
"""
import numpy as np

# (the camera rows [V, 15] float64, P row-major | centre, and the projection of points by one row)
from appearance_truth import pack_cameras, plane_scene, project_points  # noqa: F401

F = np.float32
D = np.float64

FLOATER = (slice(10, 14), slice(14, 18))        # view 0, depth x 0.7
DENT = (slice(3, 6), slice(20, 24))             # view 0, depth x 1.2


def check_points(points, cameras, depths, exclude, tol_abs, tol_rel, border, swap_signs=False,
                 skip_exclude=True):
    """points [3, n] f64; cameras [V, 15] f64; depths [V, H, W] f32; exclude: a view or -1 ->
    (seen [n] u32, agree [n] u32, violate [n] u32, residual [n] f32).  swap_signs and
    skip_exclude=False are the two mutants of tests/test_consistency_truth.py: the violate and the
    occluded tests exchanged, and the excluded view asked like the others."""
    p = np.asarray(points, D).reshape(3, -1)
    x, y, z = p[0], p[1], p[2]
    n = p.shape[1]
    cameras = np.asarray(cameras, D).reshape(-1, 15)
    depths = np.asarray(depths, F)
    V, H, W = depths.shape
    assert len(cameras) == V and 1 <= V <= 32 and -1 <= exclude < V
    tol_abs, tol_rel, border = D(tol_abs), D(tol_rel), D(border)
    seen, agree, violate = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    num, cnt = np.zeros(n, D), np.zeros(n, D)
    with np.errstate(all="ignore"):
        x_max, y_max = D(W - 1) - border, D(H - 1) - border
        for v in range(V):
            if skip_exclude and v == exclude:
                continue
            X, Y, _, _, _, dd, ok = project_points(cameras[v], x, y, z, border, x_max, y_max)
            # a view that is not in view reads pixel (0, 0)
            xi = np.rint(np.where(ok, X, 0.0)).astype(np.int64)
            yi = np.rint(np.where(ok, Y, 0.0)).astype(np.int64)
            zm = depths[v][yi, xi].astype(D)
            measured = ok & (zm > 0) & (zm < np.inf)
            s = (zm * zm - dd) / (zm + zm)
            t = tol_abs + tol_rel * zm
            agrees = measured & (s >= -t) & (s <= t)
            violates = measured & ((s < -t) if swap_signs else (s > t))
            bit = np.uint32(1 << v)
            seen = np.where(measured, seen | bit, seen).astype(np.uint32)
            agree = np.where(agrees, agree | bit, agree).astype(np.uint32)
            violate = np.where(violates, violate | bit, violate).astype(np.uint32)
            num = np.where(agrees, num + s, num)
            cnt = np.where(agrees, cnt + 1.0, cnt)
        residual = np.where(cnt > 0, (num / cnt).astype(F), F(0.0)).astype(F)
    return seen, agree, violate, residual


def popcount(mask):
    """The number of set bits of every uint32, by shifting."""
    m = np.asarray(mask, np.uint32).astype(np.uint64)
    return sum(((m >> k) & 1) for k in range(32)).astype(np.uint8)


def keep(depth, agree, violate, min_views=2, max_violations=0):
    """The pixels (or points) that stay: they hold a measurement themselves, at least min_views
    views agree and at most max_violations see past them."""
    depth = np.asarray(depth, F)
    with np.errstate(invalid="ignore"):
        measured = (depth > 0) & (depth < np.inf)
    return measured & (popcount(agree) >= min_views) & (popcount(violate) <= max_violations)


# ------------------------------------------------------------------------------- the inputs
def back_project(cam, depth):
    """[3, H*W] f64: the point every pixel of a PlaneCamera's map sees at its depth, row-major
    (pixel (Y, X) at column Y*W + X); analytic, from the camera's own numbers."""
    H, W = depth.shape
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    d = np.stack([(X - cam.u0) / cam.focal, (Y - cam.v0) / cam.focal, -np.ones_like(X)])
    d = d / np.sqrt((d * d).sum(0))
    c = np.array([cam.cx, cam.cy, cam.height], D)
    return (c[:, None, None] + depth.astype(D) * d).reshape(3, H * W)


def pinv_and_centre(cam):
    """(P_pinv [4, 3], centre [4]) of a PlaneCamera, as rn_depthmap_points takes them."""
    return np.linalg.pinv(np.asarray(cam.P, D)), np.array([cam.cx, cam.cy, cam.height, 1.0], D)


def perturbed_plane_scene():
    """appearance_truth.plane_scene() -- three cameras over z = 0, height 3, focal 20, 24 x 32 --
    with a floater and a dent planted in view 0 -> (cameras, rows [3, 15], depths [3, 24, 32] f32,
    kind [24, 32]: 0 untouched, 1 floater, 2 dent)."""
    cams, _, depths = plane_scene()
    depths = depths.copy()
    depths[0][FLOATER] = (depths[0][FLOATER] * F(0.7)).astype(F)
    depths[0][DENT] = (depths[0][DENT] * F(1.2)).astype(F)
    kind = np.zeros(depths[0].shape, np.int64)
    kind[FLOATER] = 1
    kind[DENT] = 2
    return cams, pack_cameras(cams), depths, kind
