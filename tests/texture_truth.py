"""The texture atlas, rn_texture_bake and rn_texture_sample restated in NumPy by brute force over
the texels (the definitions are in include/raynet_hip.h) -- the truth the GPU
kernels are held to bit for bit.

The layout is integer arithmetic.  Everything else is np.float64, one ufunc per operation and in
the definition's order (NumPy fuses nothing), vectorised over the texels per view.  The per-view
step is rn_project_colors's, written out again here on a float64 point and normal (the texel's
point is not rounded to float32, so appearance_truth.project_colors, which takes float32 points,
cannot serve).  Nothing here is taken from the kernels.
"""
import numpy as np

F = np.float32
D = np.float64
I = np.int32


# ------------------------------------------------------------------------------- the layout
class Layout(object):
    """T steps per leg, cells of S = T + 5 texels, Cw cells per row -> cells, rows, Wt, Ht."""
    __slots__ = ("nf", "T", "S", "Cw", "cells", "rows", "Wt", "Ht")

    def __init__(self, nf, T, Cw=None):
        assert nf >= 0 and 1 <= T <= 1024
        self.nf, self.T, self.S = int(nf), int(T), int(T) + 5
        self.cells = (self.nf + 1) // 2
        if Cw is None:          # the smallest Cw >= 1 with Cw Cw >= cells, by whole numbers
            Cw = 1
            while Cw * Cw < self.cells:
                Cw += 1
        assert Cw >= 1
        self.Cw = int(Cw)
        self.rows = (self.cells + self.Cw - 1) // self.Cw
        self.Wt, self.Ht = self.Cw * self.S, self.rows * self.S


def owners(L):
    """-> (face [Ht, Wt] int64 with -1 for an empty texel, i, j [Ht, Wt] the texel within its cell,
    lower [Ht, Wt] bool)."""
    ty, tx = np.mgrid[0:L.Ht, 0:L.Wt].astype(np.int64)
    cx, i, cy, j = tx // L.S, tx % L.S, ty // L.S, ty % L.S
    lower = i + j <= L.T + 3
    f = 2 * (cy * L.Cw + cx) + np.where(lower, 0, 1)
    return np.where(f < L.nf, f, -1), i, j, lower


def corner_texels(L, f):
    """[3, 2] whole atlas coordinates (x, y) of the corners p0, p1, p2 of face f's chart."""
    T, k = L.T, f // 2
    x, y = (k % L.Cw) * L.S, (k // L.Cw) * L.S
    if f % 2 == 0:
        local = [(1, 1), (T + 1, 1), (1, T + 1)]
    else:
        local = [(T + 3, T + 3), (3, T + 3), (T + 3, 3)]
    return np.array([(x + a, y + b) for a, b in local], np.int64)


def atlas_position(L, f, u, v):
    """The atlas position (x, y) float64 of the barycentrics (u, v) of faces f (arrays)."""
    f = np.asarray(f, np.int64)
    U, Vb = np.asarray(u, D), np.asarray(v, D)
    lower, k = f % 2 == 0, f // 2
    T = D(L.T)
    a = np.where(lower, 1.0 + U * T, D(L.T + 3) - U * T)
    b = np.where(lower, 1.0 + Vb * T, D(L.T + 3) - Vb * T)
    return ((k % L.Cw) * L.S).astype(D) + a, ((k // L.Cw) * L.S).astype(D) + b


def footprint(L, f, u, v, bilinear=True):
    """The texels [(x, y)] that carry non-zero weight in the lookup of one point."""
    x, y = (float(c) for c in atlas_position(L, f, u, v))
    if not bilinear:
        return [(int(np.rint(x)), int(np.rint(y)))]
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    x1, y1 = min(x0 + 1, L.Wt - 1), min(y0 + 1, L.Ht - 1)
    fx, fy = x - x0, y - y0
    out = []
    for (tx, wx) in ((x0, 1.0 - fx), (x1, fx)):
        for (ty, wy) in ((y0, 1.0 - fy), (y1, fy)):
            if wx != 0 and wy != 0:
                out.append((tx, ty))
    return out


def face_uvs(L):
    """(nf, 3, 2) float64: ((x + 0.5) / Wt, 1 - (y + 0.5) / Ht) at the three corners."""
    out = np.zeros((L.nf, 3, 2), D)
    for f in range(L.nf):
        c = corner_texels(L, f).astype(D)
        out[f, :, 0] = (c[:, 0] + 0.5) / L.Wt
        out[f, :, 1] = 1.0 - (c[:, 1] + 0.5) / L.Ht
    return out


# ------------------------------------------------------------------------------- the bake
def texel_points(vertices, faces, L, normals=None):
    """Per texel of the atlas -> (known [Ht, Wt] bool: a face owns it and names three vertices,
    point [Ht, Wt, 3] f64, normal [Ht, Wt, 3] f64 -- not normalised --, u, v [Ht, Wt] f64 after
    the clamp onto the triangle).  Rows of texels that are not known hold zeros."""
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, I).reshape(-1, 3)
    nv = len(vertices)
    assert len(faces) == L.nf
    face, i, j, lower = owners(L)
    idx = faces[np.where(face >= 0, face, 0)].astype(np.int64) if L.nf else \
        np.zeros(face.shape + (3,), np.int64)
    known = (face >= 0) & ((idx >= 0) & (idx < nv)).all(-1)
    idx = np.where(known[..., None], idx, 0)
    T = D(L.T)
    u0 = np.where(lower, (i - 1).astype(D) / T, ((L.T + 3) - i).astype(D) / T)
    v0 = np.where(lower, (j - 1).astype(D) / T, ((L.T + 3) - j).astype(D) / T)
    u, v = np.where(u0 > 0, u0, 0.0), np.where(v0 > 0, v0, 0.0)
    s = u + v
    over = s > 1
    with np.errstate(all="ignore"):
        u, v = np.where(over, u / s, u), np.where(over, v / s, v)
        Wb = (1.0 - u) - v
        P = vertices.astype(D) if nv else np.zeros((1, 3), D)
        p0, p1, p2 = P[idx[..., 0]], P[idx[..., 1]], P[idx[..., 2]]
        mix = lambda a0, a1, a2: (Wb[..., None] * a0 + u[..., None] * a1) + v[..., None] * a2
        point = mix(p0, p1, p2)
        if normals is not None:
            N = np.ascontiguousarray(normals, F).reshape(-1, 3).astype(D)
            normal = mix(N[idx[..., 0]], N[idx[..., 1]], N[idx[..., 2]])
        else:
            e1, e2 = p1 - p0, p2 - p0
            normal = np.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1],
                               e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                               e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], -1)
    zero = ~known[..., None]
    return known, np.where(zero, 0.0, point), np.where(zero, 0.0, normal), u, v


def project(points, normal, cameras, images, depths, tol, min_cos, border, mode):
    """rn_project_colors's definition on float64 points [n, 3] and normals [n, 3] (a zero normal:
    no facing test, weight 1) -> (colors [n, C] f32, weight [n] f32, views [n] uint32)."""
    p = np.asarray(points, D).reshape(-1, 3)
    nr = np.asarray(normal, D).reshape(-1, 3)
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
            cam = cameras[v]
            h = [((cam[4 * k] * x + cam[4 * k + 1] * y) + cam[4 * k + 2] * z) + cam[4 * k + 3]
                 for k in range(3)]
            X, Y = h[0] / h[2], h[1] / h[2]
            dx, dy, dz = cam[12] - x, cam[13] - y, cam[14] - z
            dd = (dx * dx + dy * dy) + dz * dz
            ok = (h[2] > 0) & (h[2] < np.inf) & (dd > 0) & (X >= border) & (X <= x_max) & \
                (Y >= border) & (Y <= y_max)
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
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            img = images[v].astype(D)
            i00, i01, i10, i11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
            top = i00 + fx[:, None] * (i01 - i00)
            bot = i10 + fx[:, None] * (i11 - i10)
            col = top + fy[:, None] * (bot - top)
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


def bake(vertices, faces, L, cameras, images, depths=None, normals=None, tol=0.0, min_cos=0.0,
         border=0.0, mode=0):
    """-> (texture [Ht, Wt, C] f32, weight [Ht, Wt] f32, views [Ht, Wt] uint32).  cameras [V, 15]
    f64 rows P | centre, images [V, H, W, C] f32, depths [V, H, W] f32 or None, normals [nv, 3] f32
    or None (the face's e1 x e2), mode 0 blend / 1 best."""
    images = np.asarray(images, F)
    C = images.shape[3]
    known, point, normal, _, _ = texel_points(vertices, faces, L, normals)
    colors, weight, views = project(point.reshape(-1, 3), normal.reshape(-1, 3), cameras, images,
                                    depths, tol, min_cos, border, mode)
    k = known.reshape(-1)
    texture = np.where(k[:, None], colors, F(0)).astype(F).reshape(L.Ht, L.Wt, C)
    weight = np.where(k, weight, F(0)).astype(F).reshape(L.Ht, L.Wt)
    views = np.where(k, views, np.uint32(0)).astype(np.uint32).reshape(L.Ht, L.Wt)
    return texture, weight, views


# ------------------------------------------------------------------------------- the lookup
def sample(face, bary, L, texture, bilinear=True):
    """face [...] i32, bary [..., 2] f32 -> [..., C] f32: the atlas at (u, v) of the face's chart,
    0 for a face outside [0, nf) and for u or v outside [0, 1] (a NaN is)."""
    texture = np.asarray(texture, F)
    assert texture.shape[:2] == (L.Ht, L.Wt)
    C = texture.shape[2]
    shape = np.shape(face)
    f = np.asarray(face, np.int64).reshape(-1)
    b = np.asarray(bary, F).reshape(-1, 2)
    U, Vb = b[:, 0].astype(D), b[:, 1].astype(D)
    with np.errstate(all="ignore"):
        known = (f >= 0) & (f < L.nf) & (U >= 0) & (U <= 1) & (Vb >= 0) & (Vb <= 1)
    f, U, Vb = np.where(known, f, 0), np.where(known, U, 0.0), np.where(known, Vb, 0.0)
    if L.nf == 0:
        return np.zeros(shape + (C,), F)
    x, y = atlas_position(L, f, U, Vb)
    tex = texture.astype(D)
    if bilinear:
        xf, yf = np.floor(x), np.floor(y)
        fx, fy = x - xf, y - yf
        x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, L.Wt - 1), np.minimum(y0 + 1, L.Ht - 1)
        t00, t01, t10, t11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
        top = t00 + fx[:, None] * (t01 - t00)
        bot = t10 + fx[:, None] * (t11 - t10)
        out = (top + fy[:, None] * (bot - top)).astype(F)
    else:
        out = texture[np.rint(y).astype(np.int64), np.rint(x).astype(np.int64)]
    return np.where(known[:, None], out, F(0)).astype(F).reshape(shape + (C,))
