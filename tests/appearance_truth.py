"""Vertex normals and projected colours, restated in NumPy (DESIGN.md section 20,
include/raynet_hip.h: rn_vertex_area_normals / rn_project_colors): the definitions the GPU tests
hold the kernels to bit for bit.

Everything is np.float64 arithmetic, one ufunc per operation and in the definition's order (NumPy
fuses nothing), vectorised over the points per view, and over the vertices per k-th incident face
for the normals.  Nothing here is taken from the kernels.
"""
import numpy as np

F = np.float32
D = np.float64


# ------------------------------------------------------------------------------- the normals
def corner_table(faces, nv):
    """(offsets [nv + 1] int32, corners [3 nf] int32): the corners c = 3 face + slot sorted by the
    vertex they name, ascending c within a vertex; the exclusive prefix of the corner counts."""
    flat = np.asarray(faces, np.int64).reshape(-1)
    corners = np.argsort(flat, kind="stable").astype(np.int32)
    counts = np.bincount(flat, minlength=nv)
    offsets = np.zeros(nv + 1, np.int64)
    offsets[1:] = np.cumsum(counts)
    return offsets.astype(np.int32), corners


def area_normals(vertices, faces, offsets=None, corners=None):
    """[nv, 3] float32: per vertex the sum, in the order of its row of the corner table, of
    e1 x e2 of the faces the row names, in float64, rounded once to float32 at the end.  A slot k
    outside [0, 3 nf), a corner outside [0, 3 nf) and a face with a vertex outside [0, nv) are
    skipped."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nv, nf = len(vertices), len(faces)
    if offsets is None:
        offsets, corners = corner_table(faces, nv)
    offsets = np.asarray(offsets, np.int64)
    corners = np.asarray(corners, np.int64)
    first = np.clip(offsets[:-1], 0, 3 * nf)
    last = np.clip(offsets[1:], 0, 3 * nf)
    s = np.zeros((nv, 3), D)
    P = vertices.astype(D)
    k = 0
    while True:
        live = np.nonzero(first + k < last)[0]
        if not len(live):
            break
        c = corners[first[live] + k]
        ok = (c >= 0) & (c < 3 * nf)
        live, c = live[ok], c[ok]
        idx = faces[c // 3].astype(np.int64)
        ok = ((idx >= 0) & (idx < nv)).all(1)
        live, idx = live[ok], idx[ok]
        p0, p1, p2 = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
        e1, e2 = p1 - p0, p2 - p0
        a = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        s[live] = s[live] + a
        k += 1
    return s.astype(F)


def valence(faces, nv):
    return np.bincount(np.asarray(faces, np.int64).reshape(-1), minlength=nv)


# ------------------------------------------------------------------------------- the colours
def pack_cameras(cameras):
    """[V, 15] float64: P (3 x 4, row-major) | centre [3]."""
    rows = np.empty((len(cameras), 15), D)
    for row, cam in zip(rows, cameras):
        row[:12] = np.asarray(cam.P, D).reshape(12)
        row[12:] = np.asarray(cam.center, D).reshape(-1)[:3]
    return rows


def bilerp(i00, i01, i10, i11, fx, fy):
    """The four neighbours i<row><column> at the fractions (fx, fy): along x first, then y."""
    top = i00 + fx * (i01 - i00)
    bot = i10 + fx * (i11 - i10)
    return top + fy * (bot - top)


def project_points(cam, x, y, z, border, x_max, y_max):
    """One camera row and float64 points -> (X, Y, dx, dy, dz, dd, ok): the pixel, the vector to
    the centre, its squared length, and whether the point lies in front of the camera, off its
    centre and inside the image less the border.  (Under np.errstate(all="ignore").)"""
    h = [((cam[4 * k] * x + cam[4 * k + 1] * y) + cam[4 * k + 2] * z) + cam[4 * k + 3]
         for k in range(3)]
    X, Y = h[0] / h[2], h[1] / h[2]
    dx, dy, dz = cam[12] - x, cam[13] - y, cam[14] - z
    dd = (dx * dx + dy * dy) + dz * dz
    ok = (h[2] > 0) & (h[2] < np.inf) & (dd > 0) & (X >= border) & (X <= x_max) & \
        (Y >= border) & (Y <= y_max)
    return X, Y, dx, dy, dz, dd, ok


def observe(points, normals, cameras, images, depths, tol, min_cos, border, mode):
    """The per-view step of the definition, stated once: points [n, 3] f64, normals [n, 3] f64 or
    None (as a zero normal: no facing test, weight 1), cameras [V, 15] f64, images [V, H, W, C]
    f32, depths [V, H, W] f32 or None, mode 0 / 1 -> (colors [n, C] f32, weight [n] f32,
    views [n] uint32)."""
    p = np.asarray(points, D).reshape(-1, 3)
    nr = np.zeros_like(p) if normals is None else np.asarray(normals, D).reshape(-1, 3)
    n = len(p)
    cameras = np.asarray(cameras, D).reshape(-1, 15)
    images = np.asarray(images, F)
    V, H, W, C = images.shape
    assert len(cameras) == V and 1 <= C <= 4 and 0 <= V <= 32
    tol, min_cos, border = D(tol), D(min_cos), D(border)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        nx, ny, nz = nr[:, 0], nr[:, 1], nr[:, 2]
        nn = (nx * nx + ny * ny) + nz * nz
        facing = nn > 0
        mc2 = min_cos * min_cos
        x_max, y_max = D(W - 1) - border, D(H - 1) - border
        num, best = np.zeros((n, C), D), np.zeros((n, C), D)
        den, best_w = np.zeros(n, D), np.full(n, -1.0, D)
        seen = np.zeros(n, np.uint32)
        for v in range(V):
            X, Y, dx, dy, dz, dd, ok = project_points(cameras[v], x, y, z, border, x_max, y_max)
            dot = (nx * dx + ny * dy) + nz * dz
            q = nn * dd
            dot2 = dot * dot
            ok = ok & (~facing | ((dot > 0) & (dot2 > mc2 * q)))
            w = np.where(facing, dot2 / q, 1.0)
            Xs, Ys = np.where(ok, X, 0.0), np.where(ok, Y, 0.0)
            if depths is not None:
                zf = np.asarray(depths, F)[v][np.rint(Ys).astype(np.int64),
                                              np.rint(Xs).astype(np.int64)]
                lim = zf.astype(D) + tol
                ok = ok & (zf > 0) & (dd <= lim * lim)
            xf, yf = np.floor(Xs), np.floor(Ys)
            fx, fy = Xs - xf, Ys - yf
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            # (the coordinates of a view that stopped counting at the occlusion test are its own)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            img = images[v].astype(D)
            col = bilerp(img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1],       # [n, C]
                         fx[:, None], fy[:, None])
            seen = np.where(ok, seen | np.uint32(1 << v), seen).astype(np.uint32)
            den = np.where(ok, den + w, den)
            num = np.where(ok[:, None], num + w[:, None] * col, num)
            better = ok & (w > best_w)
            best_w = np.where(better, w, best_w)
            best = np.where(better[:, None], col, best)
        blend = num / den[:, None]
        out = (blend if mode == 0 else best).astype(F)
        colors = np.where((seen != 0)[:, None], out, F(0)).astype(F)
    return colors, den.astype(F), seen


def project_colors(points, normals, cameras, images, depths, tol, min_cos, border, mode):
    """rn_project_colors: points [n, 3] f32 and normals [n, 3] f32 or None, widened to float64;
    the rest is observe's."""
    return observe(np.asarray(points, F).reshape(-1, 3).astype(D),
                   None if normals is None else np.asarray(normals, F).reshape(-1, 3).astype(D),
                   cameras, images, depths, tol, min_cos, border, mode)


# ------------------------------------------------------------------------------- the inputs
class PlaneCamera(object):
    """A camera at (cx, cy, height) looking straight down the z axis at the plane z = 0: pixel
    (X, Y) of the point (x, y, z) is (focal (x - cx) / (height - z) + u0, focal (y - cy) /
    (height - z) + v0)."""

    def __init__(self, cx, cy, height, focal, u0, v0):
        self.cx, self.cy, self.height, self.focal, self.u0, self.v0 = cx, cy, height, focal, u0, v0
        # h = (focal (x - cx) + u0 (height - z), focal (y - cy) + v0 (height - z), height - z)
        self.P = np.array([[focal, 0.0, -u0, -focal * cx + u0 * height],
                           [0.0, focal, -v0, -focal * cy + v0 * height],
                           [0.0, 0.0, -1.0, height]], D)
        self.center = np.array([[cx], [cy], [height], [1.0]], F)

    def ground_point(self, X, Y):
        """The point of the plane z = 0 that pixel (X, Y) sees."""
        return (X - self.u0) * self.height / self.focal + self.cx, \
            (Y - self.v0) * self.height / self.focal + self.cy


def affine_field(x, y, C=3):
    """A colour field over the plane that is affine in (x, y), within [0, 1] for |x|, |y| <= 3."""
    coef = np.array([[0.5, 0.07, 0.05], [0.4, -0.06, 0.03], [0.6, 0.02, -0.08], [0.3, 0.05, 0.05]], D)
    return np.stack([coef[c, 0] + coef[c, 1] * x + coef[c, 2] * y for c in range(C)], -1)


def plane_scene(H=24, W=32, focal=20.0, height=3.0, C=3,
                centres=((-0.35, 0.1), (0.3, -0.2), (0.05, 0.45))):
    """Three translated cameras over the plane z = 0 that carries `affine_field`: (cameras,
    images [V, H, W, C] f32, depths [V, H, W] f32), images and depth maps computed analytically
    (a pixel's colour is the field at the ground point it sees; its depth the distance of that
    point to the camera centre)."""
    cams = [PlaneCamera(cx, cy, height, focal, (W - 1) / 2.0, (H - 1) / 2.0) for cx, cy in centres]
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    images, depths = [], []
    for cam in cams:
        gx, gy = cam.ground_point(X, Y)
        images.append(affine_field(gx, gy, C).astype(F))
        depths.append(np.sqrt((gx - cam.cx) ** 2 + (gy - cam.cy) ** 2 + height ** 2).astype(F))
    return cams, np.stack(images), np.stack(depths)


def tetrahedron():
    """A regular tetrahedron, faces counter-clockwise seen from outside."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def constant_camera(x, y, h2, centre):
    """A camera row that sends every point to pixel (x, y) at h_2 = h2."""
    return np.array([0, 0, 0, x * h2, 0, 0, 0, y * h2, 0, 0, 0, h2] + list(centre), D)


def planted_scene():
    """Points, depths and normals planted on the edges of the definition, 24 x 32 x 3 images.
    View 0 (and its copy, view 1) looks straight down from (0, 0, 4) with focal 16 and principal
    point (8, 8): a point of the plane z = 0 lands at (4 x + 8, 4 y + 8), exactly.  View 2 sends
    every point to X = 31, the last column, view 3 to one fp64 step beyond it; view 4 has its
    centre AT one of the points."""
    H, W, C = 24, 32, 3
    cam = PlaneCamera(0.0, 0.0, 4.0, 16.0, 8.0, 8.0)
    beyond = np.nextafter(31.0, np.inf)
    cameras = np.stack([pack_cameras([cam])[0], pack_cameras([cam])[0],
                        constant_camera(31.0, 8.0, 4.0, (0, 0, 4)),
                        constant_camera(beyond, 8.0, 1.0, (0, 0, 4)),
                        constant_camera(5.0, 5.0, 1.0, (0.25, 0.5, 0.75))])
    assert cameras[3, 3] > 31.0 and cameras[3, 3] / cameras[3, 11] == beyond
    names, pts, nrm = [], [], []

    def plant(name, p, normal=(0, 0, 0)):
        names.append(name)
        pts.append(p)
        nrm.append(normal)

    plant("behind the camera", (0, 0, 5))
    plant("on the camera plane", (1, 0, 4))
    plant("at the centre of views 0-3", (0, 0, 4))
    plant("at the centre of view 4", (0.25, 0.5, 0.75))
    plant("X = 0", (-2, 0, 0))
    plant("X = W - 1", (5.75, 0, 0))
    plant("X = 0.5", (-1.875, 0, 0))
    plant("X = 1.5", (-1.625, 0, 0))
    plant("X = 2.5", (-1.375, 0, 0))
    plant("NaN", (np.nan, 0, 0))
    plant("inf", (0, np.inf, 0))
    for k, name in enumerate(("depth 0", "depth negative", "depth NaN", "depth inf")):
        plant(name, ((10 + k - 8) / 4.0, 0, 0))
    plant("zero normal", (0.5, 0.5, 0), (0, 0, 0))
    plant("facing away", (0.5, 0.5, 0), (0, 0, -1))
    plant("perpendicular", (0, 0, 0), (1, 0, 0))
    plant("facing", (0, 0, 0), (0, 0, 2))
    rng = np.random.default_rng(3)
    images = rng.random((5, H, W, C)).astype(F)
    depths = np.full((5, H, W), np.inf, F)
    depths[:2, 8, [1, 3]] = 0               # X = 0.5 / 2.5 rounded away from even would hit these
    depths[:2, 8, 10:14] = np.array([0, -1, np.nan, np.inf], F)
    return dict(names=names, points=np.array(pts, F), normals=np.array(nrm, F), cameras=cameras,
                images=images, depths=depths)


def check_planted(got, scene, mode):
    """What the definition says about planted_scene's points, worked out by hand: `got` =
    (colors, weight, views) of a run with tol = min_cos = border = 0 in `mode`."""
    colors, weight, views = got
    names, images = scene["names"], scene["images"]
    at_ = {name: k for k, name in enumerate(names)}

    def sees(view, name):
        return bool((views[at_[name]] >> view) & 1)

    # views 0 and 1, the real camera: h_2 <= 0, dd = 0 and non-finite coordinates see nothing
    for name in ("behind the camera", "on the camera plane", "at the centre of views 0-3", "NaN",
                 "inf", "depth 0", "depth negative", "depth NaN", "facing away", "perpendicular"):
        assert not sees(0, name) and not sees(1, name), name
    for name in ("X = 0", "X = W - 1", "X = 0.5", "X = 1.5", "X = 2.5", "depth inf",
                 "zero normal", "facing", "at the centre of view 4"):
        assert sees(0, name) and sees(1, name), name
    # a NaN coordinate makes dd NaN, an infinite one makes 0 * inf = NaN of the constant cameras'
    # h: no view at all, and the row is exactly +0
    for k in (at_["NaN"], at_["inf"]):
        assert views[k] == 0 and weight[k] == 0 and (colors[k] == 0).all()
        assert not np.signbit(colors[k]).any() and not np.signbit(weight[k])
    # views 2 and 3 have their centre at (0, 0, 4): dd = 0 there
    assert not sees(2, "at the centre of views 0-3") and not sees(3, "at the centre of views 0-3")
    for name in names:
        assert not sees(3, name), name                          # one step beyond W - 1: nobody
    for name in ("X = 0", "X = W - 1", "depth 0", "zero normal", "facing", "behind the camera"):
        assert sees(2, name), name                              # exactly W - 1: in view
    assert not sees(2, "perpendicular") and not sees(2, "facing away") and not sees(2, "NaN")
    # view 4 has its centre at one of the points
    assert not sees(4, "at the centre of view 4") and sees(4, "at the centre of views 0-3")
    assert sees(4, "zero normal") and not sees(4, "facing away") and sees(4, "perpendicular")
    if mode == 1:
        # exactly on a column: the pixel itself; view 0 is the first of the views of weight 1
        assert np.array_equal(colors[at_["X = 0"]], images[0, 8, 0])
        assert np.array_equal(colors[at_["X = W - 1"]], images[0, 8, 31])
        # a tie: views 0 and 1 are the same camera, cos^2 = 1 in both; the first wins
        assert np.array_equal(colors[at_["facing"]], images[0, 8, 8])
        assert not np.array_equal(images[0, 8, 8], images[1, 8, 8])
    # cos^2 = 1 from views 0, 1 and 2, 1.5^2 / (4 * 0.875) from view 4
    assert weight[at_["facing"]] == F(3.0 + 2.25 / 3.5)
    assert weight[at_["zero normal"]] == 4 and weight[at_["X = 0"]] == 4
