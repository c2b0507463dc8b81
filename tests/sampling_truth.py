"""sample_in_range and sample_in_disparity (include/raynet_hip.h, "sampling schemes"; DESIGN.md
section 17) restated in NumPy, operation by operation, and the plane sweep's similarity on any
set of per-plane points.

The float32 / float64 split is the kernels': the ray of a pixel is sample_in_bbox's (fp64
back-projection, `dir` rounded to fp32 once), sample_in_range is fp32 throughout with every
operation rounded on its own, sample_in_disparity is fp64 from the fp32 ends of the box segment
on and rounds the point to fp32 once.  The GPU tests ask the kernels for these bits (range: the
bbox test's bound, its square root is the one operation NumPy and the device need not share).
"""
import numpy as np

from batch_truth import sample_in_bbox_f32

f32, f64 = np.float32, np.float64


def pixel_ray_f32(ri, H, Pinv, cc):
    """raynet_kernels.h pixel_ray: Pinv [n, 4, 3] f32, cc [n, 4] f32 -> dir [n, 3] f32."""
    ri = np.asarray(ri, np.int64)
    px, py = (ri // H).astype(f32), (ri % H).astype(f32)
    o = np.zeros((len(ri), 4), f64)
    for r in range(4):
        a = np.zeros(len(ri), f64)
        a = a + (Pinv[:, r, 0] * px).astype(f64)
        a = a + (Pinv[:, r, 1] * py).astype(f64)
        a = a + Pinv[:, r, 2].astype(f64) * 1.0
        o[:, r] = a
    return np.stack([(o[:, i] / o[:, 3] - cc[:, i].astype(f64)).astype(f32) for i in range(3)], 1)


def _per_ray(n, Pinv, cc):
    Pinv, cc = np.asarray(Pinv, f32), np.asarray(cc, f32)
    Pinv = np.broadcast_to(Pinv.reshape(-1, 4, 3), (n, 4, 3))
    cc = np.broadcast_to(cc.reshape(-1, cc.shape[-1]), (n, cc.shape[-1]))
    return Pinv, cc


def plane_points_f32(s, e, D):
    """plane_point(s, e, k, D) for k = 0 .. D-1: [n, D, 3] f32."""
    k = np.arange(D).astype(f32)[None, :, None]
    pts = s[:, None, :] + k * (e - s)[:, None, :] / f32(D - 1)
    assert pts.dtype == f32
    return pts


def range_segment_f32(ri, H, Pinv, cc, depth_range):
    """-> s, e [n, 3] f32: centre + r0 d^, centre + r1 d^."""
    n = len(ri)
    Pinv, cc = _per_ray(n, Pinv, cc)
    d = pixel_ray_f32(ri, H, Pinv, cc)
    r0, r1 = f32(depth_range[0]), f32(depth_range[1])
    with np.errstate(all="ignore"):
        norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        dh = [d[:, i] / norm for i in range(3)]
        s = np.stack([cc[:, i] + r0 * dh[i] for i in range(3)], 1)
        e = np.stack([cc[:, i] + r1 * dh[i] for i in range(3)], 1)
    assert s.dtype == f32 and e.dtype == f32
    return s, e


def sample_in_range(ri, H, Pinv, cc, depth_range, D):
    """-> points [n, D, 4] f32 (w = 1)."""
    s, e = range_segment_f32(ri, H, Pinv, cc, depth_range)
    pts = plane_points_f32(s, e, D)
    return np.concatenate([pts, np.ones(pts.shape[:2] + (1,), f32)], 2)


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def sample_in_disparity(ri, H, Pinv, cc, bbox, far_cam, D):
    """far_cam [28] or [n, 28] f32 (P_pinv 4x3 | centre 4 | P 3x4) -> dict(points [n, D, 4] f32,
    missed [n] bool, parallel [n, D] f64 = 1 - (a1.a2)^2 / ((a1.a1)(a2.a2))).  A missed ray: the
    camera centre D times with w = 0."""
    ri = np.asarray(ri, np.int64)
    n = len(ri)
    Pinv, cc = _per_ray(n, Pinv, cc)
    bbox = np.asarray(bbox, f32).ravel()
    far = np.broadcast_to(np.asarray(far_cam, f32).reshape(-1, 28), (n, 28))
    with np.errstate(all="ignore"):
        d = pixel_ray_f32(ri, H, Pinv, cc)
        s, e, missed = sample_in_bbox_f32(ri, H, Pinv, cc, bbox)
        P = far[:, 16:].reshape(n, 3, 4).astype(f64)
        pix = []
        for x in (s.astype(f64), e.astype(f64)):
            q = [((P[:, r, 0] * x[:, 0] + P[:, r, 1] * x[:, 1]) + P[:, r, 2] * x[:, 2]) + P[:, r, 3]
                 for r in range(3)]
            pix.append((np.rint(q[0] / q[2]), np.rint(q[1] / q[2])))
        u0, v0 = pix[0]
        du, dv = pix[1][0] - pix[0][0], pix[1][1] - pix[0][1]
        c1 = [cc[:, i].astype(f64) for i in range(3)]
        a1 = [d[:, i].astype(f64) for i in range(3)]
        c2 = [far[:, 12 + i].astype(f64) for i in range(3)]
        a11, a1p1, a1p2 = _dot3(a1, a1), _dot3(a1, c1), _dot3(a1, c2)
        Pi = far[:, :12].reshape(n, 4, 3).astype(f64)
        t = np.linspace(0, 1, D, dtype=f32)
        assert t[-1] == 1 and np.array_equal(
            t[:-1], (np.arange(D - 1).astype(f64) * (1.0 / f64(D - 1))).astype(f32))
        points = np.zeros((n, D, 4), f32)
        parallel = np.zeros((n, D), f64)
        for k in range(D):
            pu = (u0 + f64(t[k]) * du).astype(f32).astype(f64)
            pv = (v0 + f64(t[k]) * dv).astype(f32).astype(f64)
            o = [(Pi[:, r, 0] * pu + Pi[:, r, 1] * pv) + Pi[:, r, 2] for r in range(4)]
            a2 = [o[i] / o[3] - c2[i] for i in range(3)]
            a22, a12 = _dot3(a2, a2), _dot3(a1, a2)
            a2p1, a2p2 = _dot3(a2, c1), _dot3(a2, c2)
            div = a11 * a22 - a12 * a12
            t1 = (-a22 * (a1p1 - a1p2) + a12 * (a2p1 - a2p2)) / div
            for i in range(3):
                points[:, k, i] = (c1[i] + a1[i] * t1).astype(f32)
            parallel[:, k] = 1.0 - (a12 * a12) / (a11 * a22)
        points[..., 3] = 1.0
        points[missed, :, :3] = cc[missed, None, :3]
        points[missed, :, 3] = 0.0
    return dict(points=points, missed=missed, parallel=parallel)


# ------------------------------------------------------------------ the sweep on given points
def _to_i32_sat(x):
    out = np.zeros(x.shape, np.int64)
    ok = np.isfinite(x)
    out[ok] = np.clip(x[ok].astype(f64), -2147483648.0, 2147483647.0).astype(np.int64)
    out[np.isposinf(x)] = 2147483647
    out[np.isneginf(x)] = -2147483648
    return out


def feature_pixels(points, Pv, H, W, padding):
    """feature_similarities.cu:10-61 (raynet_kernels.h feature_offset): points [n, D, 3] f32, Pv
    [3, 4] f32 -> (fy, fx) [n, D] int into the padded map."""
    X, Y, Z = points[..., 0], points[..., 1], points[..., 2]
    Pv = np.asarray(Pv, f32).reshape(3, 4)
    with np.errstate(all="ignore"):
        q = []
        for r in range(3):
            a = np.zeros(X.shape, f32)
            a = a + Pv[r, 0] * X
            a = a + Pv[r, 1] * Y
            a = a + Pv[r, 2] * Z
            a = a + Pv[r, 3] * f32(1)
            q.append(a)
        x, y = q[0] / q[2], q[1] / q[2]
        assert x.dtype == f32
        half = (padding - 1) // 2
        # roundf: half away from zero, exact in fp64 for every fp32 argument
        rx = np.sign(x) * np.floor(np.abs(x).astype(f64) + 0.5)
        ry = np.sign(y) * np.floor(np.abs(y).astype(f64) + 0.5)
        fx = _to_i32_sat((rx.astype(f32) + f32(padding) - f32(half)).astype(f32))
        fy = _to_i32_sat((ry.astype(f32) + f32(padding) - f32(half)).astype(f32))
    fx = np.minimum(np.maximum(fx, 0), W)
    fy = np.minimum(np.maximum(fy, 0), H)
    zero = (fx == 0) | (fy == 0)
    fx[zero] = 0
    fy[zero] = 0
    return fy, fx


def similarities(points, features, P, H, W, padding):
    """The plane sweep on per-plane points: projection, half-away rounding, clamp, the (0, 0)
    rule, mean over the view pairs i < j of <f_i, f_j> (serial fp32 sums in the reference's
    order), softmax over the planes.  points [n, D, 3+] f32, features [N, Hf, Wf, F] f32, P
    [N, 3, 4] f32 -> S [n, D] f32."""
    points = np.asarray(points, f32)[..., :3]
    features = np.asarray(features, f32)
    N = features.shape[0]
    P = np.asarray(P, f32).reshape(N, 3, 4)
    vec = []
    for v in range(N):
        fy, fx = feature_pixels(points, P[v], H, W, padding)
        vec.append(features[v][fy, fx])                      # [n, D, F]
    acc = np.zeros(points.shape[:2], f32)
    for i in range(N):
        for j in range(i + 1, N):
            dot = np.zeros(points.shape[:2], f32)
            for f in range(features.shape[3]):
                dot = dot + vec[i][..., f] * vec[j][..., f]
            acc = acc + dot
    acc = acc / f32(N * (N - 1) // 2)
    with np.errstate(all="ignore"):
        ex = np.exp(acc - acc.max(1, keepdims=True)).astype(f32)
        return (ex / ex.sum(1, keepdims=True, dtype=f32)).astype(f32)


# ---------------------------------------------------------------- the tests' scenes
H, W = 24, 32
RANGES = {"ring": (2.0, 4.0), "restrepo": (3.0, 7.0)}


def scene_of(kind, golden, views=5):
    """The 24 x 32 scenes of the sampling-scheme tests: the synthetic ring cameras around the box
    [-1, 1]^3, or the mock Restrepo cameras (intrinsics scaled to the image) with that scene's
    box.  Images are noise; cameras and the box are what matters."""
    import os

    from raynet_amd.common.scene import Image, Scene, restrepo_cameras_scene
    from raynet_amd.synthetic import ring_cameras
    if kind == "restrepo":
        return restrepo_cameras_scene(os.path.join(golden, "restrepo_mock_scene_1"), (H, W),
                                      n_images=views, scale=W / 1280.0)
    rng = np.random.default_rng(7)
    return Scene([Image(rng.random((H, W, 3)).astype(f32), c) for c in ring_cameras(views, H, W)],
                 (-1, -1, -1, 1, 1, 1))


def camera_arrays(scene, ref, N):
    """What K9 / K10 take for reference view `ref` with N views, and the far view's camera as the
    28 floats of a camera-table row: dict(P [N, 3, 4], P_inv [4, 3], center [4], far [28],
    views)."""
    views = scene.view_indices_with_neighbors(ref, N - 1)
    cams = [scene.get_image(v).camera for v in views]
    far = np.zeros(28, f32)
    far[:12] = np.asarray(cams[-1].P_pinv, f32).ravel()
    far[12:15] = np.asarray(cams[-1].center, f32).ravel()[:3]
    far[15] = 1.0
    far[16:] = np.asarray(cams[-1].P, f32).ravel()
    center = np.ones(4, f32)
    center[:3] = np.asarray(cams[0].center, f32).ravel()[:3]
    return dict(P=np.ascontiguousarray(np.array([c.P for c in cams], f32)),
                P_inv=np.ascontiguousarray(cams[0].P_pinv, dtype=f32), center=center, far=far,
                views=views)


def rays_with_misses(scene, ref, n, seed=0):
    """n ray indices of view `ref`: the corners and the centre first, then seeded ones."""
    rng = np.random.default_rng(seed)
    first = [0, H - 1, (W - 1) * H, W * H - 1, (W // 2) * H + H // 2]
    rest = rng.choice(H * W, max(n - len(first), 0), replace=n - len(first) > H * W)
    return np.concatenate([first, rest])[:n].astype(np.int32)
