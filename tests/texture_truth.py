"""The texture atlas, rn_texture_bake and rn_texture_sample restated in NumPy by brute force over
the texels (the definitions are in include/raynet_hip.h) -- the truth the GPU
kernels are held to bit for bit.

The layout is integer arithmetic.  Everything else is np.float64, one ufunc per operation and in
the definition's order (NumPy fuses nothing), vectorised over the texels per view.  The per-view
step is rn_project_colors's: appearance_truth.observe on the texel's float64 point and normal,
neither rounded to float32 on the way.  Nothing here is taken from the kernels.
"""
import numpy as np

import appearance_truth as at

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


def bake(vertices, faces, L, cameras, images, depths=None, normals=None, tol=0.0, min_cos=0.0,
         border=0.0, mode=0):
    """-> (texture [Ht, Wt, C] f32, weight [Ht, Wt] f32, views [Ht, Wt] uint32).  cameras [V, 15]
    f64 rows P | centre, images [V, H, W, C] f32, depths [V, H, W] f32 or None, normals [nv, 3] f32
    or None (the face's e1 x e2), mode 0 blend / 1 best."""
    images = np.asarray(images, F)
    C = images.shape[3]
    known, point, normal, _, _ = texel_points(vertices, faces, L, normals)
    colors, weight, views = at.observe(point.reshape(-1, 3), normal.reshape(-1, 3), cameras, images,
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
        out = at.bilerp(tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1], fx[:, None],
                        fy[:, None]).astype(F)
    else:
        out = texture[np.rint(y).astype(np.int64), np.rint(x).astype(np.int64)]
    return np.where(known[:, None], out, F(0)).astype(F).reshape(shape + (C,))


# ------------------------------------------------------------------------------- the inputs
def corner_scene():
    """Two faces (one cell: the lower and the upper chart) just off the plane of
    appearance_truth.plane_scene, T = 4, its three 24 x 32 x 3 views with their depth maps, vertex
    normals that lean, and no vertex or normal component equal to zero: at a chart's corner texel
    (u, v) is (0, 0), (1, 0) or (0, 1), so the texel's point and normal are the vertex's own,
    exactly (0 a + b meets no signed zero), and the bake there is rn_project_colors at the vertex."""
    cams, images, depths = at.plane_scene()
    vertices = np.array([[-0.7, -0.6, 0.02], [0.8, -0.5, -0.03], [0.75, 0.65, 0.04],
                         [-0.65, 0.7, -0.02]], F)
    faces = np.array([[0, 1, 2], [0, 2, 3]], I)
    normals = np.array([[0.1, -0.15, 1.0], [-0.2, 0.05, 0.9], [0.3, 0.25, 1.1], [-0.05, -0.3, 0.8]], F)
    assert (vertices != 0).all() and (normals != 0).all()
    return dict(vertices=vertices, faces=faces, normals=normals, L=Layout(2, 4),
                cameras=at.pack_cameras(cams), images=images, depths=depths, tol=0.1, min_cos=0.1,
                border=0.5)


def corners_of(scene, planes):
    """The rows of baked planes [Ht, Wt, ...] at the corner texels of every face, in the order
    of scene["faces"].reshape(-1)."""
    at_ = np.concatenate([corner_texels(scene["L"], f) for f in range(len(scene["faces"]))])
    return [np.asarray(p)[at_[:, 1], at_[:, 0]] for p in planes]
