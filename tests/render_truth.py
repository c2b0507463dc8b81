"""rn_mesh_render restated in NumPy by brute force (the definition is in include/raynet_hip.h;
DESIGN.md section 26) -- the truth the GPU kernel is held to bit for bit, and which
tests/test_render_truth.py ties to tests/raycast_truth.py and through it to the reference's golden.

Per pixel (column x, row y) of a view (P_pinv [4][3] f32, centre [3] f32):
  the ray is raycast_truth.pixel_rays': float64 products of the fp32 P_pinv rounded once;
  every face is tested as raycast_truth._test does, fp32 throughout, every operation rounded on its
  own, and the test's own u and v are kept; the winner has the smallest key, the lowest face on
  equal keys; the depth is the float64 distance of the hit to the centre rounded once;
  the attributes are interpolated in float64, every operation rounded on its own:
    U = f64(u), Vb = f64(v), Wb = (1 - U) - Vb, a = (Wb a0 + U a1) + Vb a2,
    a colour is f32(a); a normal n / sqrt((nx nx + ny ny) + nz nz) where that sum is > 0 and
    finite, else (0, 0, 0).
A face that names a vertex outside [0, nv) is not part of the surface (its triangle cannot be
formed); the kernel's guard for such a face is tested with triangles given apart from the faces
(`triangles=`): the hit counts, face and depth stay, the rest is 0.
"""
import numpy as np

import raycast_truth as rt

F = np.float32
D = np.float64
I = np.int32


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _test(o, ray, tri):
    """Rays [R] x triangles [T] -> (key [R, T] f32 with inf where rejected, hit xyz, u, v):
    raycast_truth._test with the barycentrics kept."""
    ox, oy, oz = (o[:, k:k + 1] for k in range(3))
    rx, ry, rz = (ray[:, k:k + 1] for k in range(3))
    p0x, p0y, p0z = (tri[None, :, k] for k in range(3))
    e1x, e1y, e1z = (tri[None, :, 3 + k] - tri[None, :, k] for k in range(3))
    e2x, e2y, e2z = (tri[None, :, 6 + k] - tri[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        px, py, pz = ry * e2z - rz * e2y, rz * e2x - rx * e2z, rx * e2y - ry * e2x
        det = _dot(e1x, e1y, e1z, px, py, pz)
        ok = ~((-rt.EPS < det) & (det < rt.EPS))
        inv = F(1) / det
        tx, ty, tz = ox - p0x, oy - p0y, oz - p0z
        u = _dot(tx, ty, tz, px, py, pz) * inv
        ok &= ~((u < 0) | (u > 1))
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        v = _dot(rx, ry, rz, qx, qy, qz) * inv
        ok &= ~((v < 0) | (u + v > 1))
        t = _dot(e2x, e2y, e2z, qx, qy, qz) * inv
        ok &= t >= 0
        hx, hy, hz = ox + t * rx, oy + t * ry, oz + t * rz
        dx, dy, dz = hx - ox, hy - oy, hz - oz
        key = _dot(dx, dy, dz, dx, dy, dz)
        ok &= key < np.inf
    key = np.where(ok, key, F(np.inf)).astype(F)
    assert u.dtype == F and v.dtype == F and key.dtype == F
    return key, hx, hy, hz, u, v


def first_hits(origins, destinations, triangles, chunk=1 << 21):
    """-> (points [R, 3] f32, face [R] i32 (-1: miss), bary [R, 2] f32, ties [R] bool: another
    triangle has the winner's key) by brute force over all triangles."""
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d = np.ascontiguousarray(destinations, F).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, F).reshape(-1, 9)
    ray = rt.normalised_rays(o, d)
    R = len(o)
    points, bary = np.zeros((R, 3), F), np.zeros((R, 2), F)
    face, ties = np.full(R, -1, I), np.zeros(R, bool)
    step = max(1, chunk // max(1, len(tri)))
    for a in range(0, R, step):
        b = min(R, a + step)
        key, hx, hy, hz, u, v = _test(o[a:b], ray[a:b], tri)
        j = np.argmin(key, axis=1)
        rows = np.arange(b - a)
        hit = key[rows, j] < np.inf
        face[a:b][hit] = j[hit]
        points[a:b][hit] = np.stack([hx[rows, j], hy[rows, j], hz[rows, j]], axis=1)[hit]
        bary[a:b][hit] = np.stack([u[rows, j], v[rows, j]], axis=1)[hit]
        ties[a:b] = hit & ((key == key[rows, j][:, None]).sum(1) > 1)
    return points, face, bary, ties


def cast(origins, destinations, triangles, centre):
    """-> (face [R] i32, depth [R] f32 (0: miss), bary [R, 2] f32, points [R, 3] f32, ties [R])
    of explicit rays: the depth is raycast_truth.depths rounded once, 0 on a miss."""
    points, face, bary, ties = first_hits(origins, destinations, triangles)
    depth = rt.depths(points, face, centre)
    depth = np.where(face >= 0, depth, 0.0).astype(F)
    return face, depth, bary, points, ties


def view_rays(camera_row, H, W):
    """Origins and destinations [H W, 3] f32 of a view's pixels, row by row."""
    row = np.asarray(camera_row, F).reshape(15)
    ys, xs = np.mgrid[0:H, 0:W]
    return rt.pixel_rays(row[:12], row[12:], xs.reshape(-1), ys.reshape(-1))


def interpolate(bary, a0, a1, a2):
    """[R, K] f64: (Wb a0 + U a1) + Vb a2 of f32 attribute rows [R, K]."""
    U, Vb = bary[:, 0:1].astype(D), bary[:, 1:2].astype(D)
    Wb = (1.0 - U) - Vb
    with np.errstate(all="ignore"):
        return (Wb * a0.astype(D) + U * a1.astype(D)) + Vb * a2.astype(D)


def unit_rows(n):
    """[R, 3] f32: n / sqrt((nx nx + ny ny) + nz nz) in f64 where that is > 0 and finite, else 0."""
    with np.errstate(all="ignore"):
        l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok = (l2 > 0) & np.isfinite(l2)
        out = n / np.sqrt(np.where(ok, l2, 1.0))[:, None]
        return np.where(ok[:, None], out, 0.0).astype(F)


class Render(object):
    __slots__ = ("face", "depth", "bary", "color", "normal", "ties")


def render(vertices, faces, cameras, H, W, colors=None, normals=None, triangles=None):
    """-> Render of face [V, H, W] i32, depth [V, H, W] f32, bary [V, H, W, 2] f32, color
    [V, H, W, C] f32 or None, normal [V, H, W, 3] f32 or None, ties [V, H, W] bool.  cameras:
    [V, 15] f32 rows P_pinv | centre.  triangles: the [nf, 9] rows the rays are cast at where they
    are not vertices[faces] (faces with indices that name no vertex)."""
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, I).reshape(-1, 3)
    cameras = np.ascontiguousarray(cameras, F).reshape(-1, 15)
    nv, V = len(vertices), len(cameras)
    known_face = ((faces >= 0) & (faces < nv)).all(1)
    if triangles is None:
        assert known_face.all()
        triangles = vertices[faces].reshape(-1, 9)
    out = Render()
    out.face, out.ties = np.full((V, H, W), -1, I), np.zeros((V, H, W), bool)
    out.depth, out.bary = np.zeros((V, H, W), F), np.zeros((V, H, W, 2), F)
    out.color = None if colors is None else np.zeros((V, H, W, np.shape(colors)[1]), F)
    out.normal = None if normals is None else np.zeros((V, H, W, 3), F)
    for k in range(V):
        o, dst = view_rays(cameras[k], H, W)
        face, depth, bary, _, ties = cast(o, dst, triangles, cameras[k, 12:])
        hit = face >= 0
        known = hit & known_face[np.where(hit, face, 0)]
        bary[~known] = 0
        corners = faces[np.where(known, face, 0)]
        corners = np.where(known[:, None], corners, 0)
        out.face[k], out.ties[k] = face.reshape(H, W), ties.reshape(H, W)
        out.depth[k], out.bary[k] = depth.reshape(H, W), bary.reshape(H, W, 2)
        if colors is not None:
            c = np.ascontiguousarray(colors, F)
            a = interpolate(bary, c[corners[:, 0]], c[corners[:, 1]], c[corners[:, 2]]).astype(F)
            out.color[k] = np.where(known[:, None], a, F(0)).reshape(H, W, -1)
        if normals is not None:
            n = np.ascontiguousarray(normals, F)
            a = unit_rows(interpolate(bary, n[corners[:, 0]], n[corners[:, 1]], n[corners[:, 2]]))
            out.normal[k] = np.where(known[:, None], a, F(0)).reshape(H, W, 3)
    return out


def camera_rows(cameras):
    """[V, 15] f32 rows P_pinv [4][3] | centre [3] of camera objects (raynet_amd.common.camera)."""
    return np.stack([np.concatenate([np.asarray(c.P_pinv, F).reshape(12),
                                     np.asarray(c.center, F).reshape(-1)[:3]]) for c in cameras])


# ------------------------------------------------------------------------------ meshes and views
DELTA = 2.0 ** -20      # how far the one triangle reaches beyond the rays through its corners


def axis_camera(size=8):
    """One camera row written by hand, exact in fp32: the centre at the origin, the pixel (x, y)
    of a size x size image looks along ((x - size/2) / size, (y - size/2) / size, 1)."""
    s, h = 1.0 / size, 0.5
    return np.array([[s, 0, -h, 0, s, -h, 0, 0, 1, 0, 0, 1, 0, 0, 0]], F)


def one_triangle():
    """-> (vertices, faces, corner pixels [(x, y)] of axis_camera(8)): a right triangle in the plane
    z = 4 whose legs reach DELTA beyond the points (-1, -1), (1, -1), (-1, 1) that the rays of the
    pixels (2, 2), (6, 2), (2, 6) pass through.  In exact arithmetic those pixels have (u, v) =
    (d, d), (1 - 3 d, d), (d, 1 - 3 d) with d = DELTA / (2 + 4 DELTA) = 4.8e-7; the fp32 test moves
    u and v by about 1e-7 there (two terms of size 2, each off by 2^-23 relative, cancel, times
    1 / det = 0.26), so all three hit."""
    L = 2 + 4 * DELTA
    p0 = np.array([-1 - DELTA, -1 - DELTA, 4])
    vertices = np.array([p0, p0 + [L, 0, 0], p0 + [0, L, 0]], F)
    return vertices, np.array([[0, 1, 2]], I), [(2, 2), (6, 2), (2, 6)]


def coincident_pair():
    """Two faces over the same three vertices' positions (six vertices, so that each face has
    colours of its own): every hit is a tie, the lower face wins."""
    v = one_triangle()[0]
    return np.concatenate([v, v]), np.array([[0, 1, 2], [3, 4, 5]], I)


def square():
    """Two triangles that share the diagonal of a square in the plane z = 4, seen head-on by
    axis_camera: the rays of the pixels with x == y run through the shared edge."""
    vertices = np.array([[-1.75, -1.75, 4], [1.75, -1.75, 4], [1.75, 1.75, 4], [-1.75, 1.75, 4]], F)
    return vertices, np.array([[0, 1, 2], [0, 2, 3]], I)


def icosphere(subdivisions=2, radius=0.6, centre=(0.0, 0.0, 0.0)):
    """A sphere of 20 * 4^subdivisions faces, counter-clockwise seen from outside."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t),
         (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4),
         (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9),
         (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, D) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.array(v) * radius + np.array(centre, D)).astype(F), np.array(f, I)


def ring_rows(V, H, W, radius=3.0, focal=None):
    """[V, 15] f32 camera rows of raynet_amd.synthetic.ring_cameras (focal: 1.5 H)."""
    from raynet_amd.synthetic import ring_cameras
    return camera_rows(ring_cameras(V, H, W, radius=radius, focal=1.5 * H if focal is None else focal))


def vertex_attributes(nv, C, seed=0):
    """Colours [nv, C] f32 in [0, 1] and unit normals [nv, 3] f32 that belong to no surface."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(nv, 3))
    return rng.random((nv, C)).astype(F), (n / np.linalg.norm(n, axis=1)[:, None]).astype(F)
