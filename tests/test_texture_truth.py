"""The restatement of the texture atlas, the bake and the lookup (tests/texture_truth.py) on its
own, without a GPU: the layout's owner table against the corner positions, the footprint property
that the constants of the layout exist for, raynet_amd.texture's host side against it, and the
bake and the lookup on scenes whose answer is known in closed form."""
import numpy as np
import pytest

import appearance_truth as at
import texture_truth as tt

F = np.float32
D = np.float64
I = np.int32
LAYOUTS = [(nf, T) for nf in range(10) for T in range(1, 6)]


def _layouts(nf, T):
    """The default layout and a few other widths."""
    seen = set()
    for Cw in (None, 1, 2, 3, 7):
        L = tt.Layout(nf, T, Cw)
        if L.Cw not in seen:
            seen.add(L.Cw)
            yield L


@pytest.mark.parametrize("nf,T", LAYOUTS)
def test_every_texel_has_one_owner_or_none_and_the_corners_are_owned(nf, T):
    for L in _layouts(nf, T):
        assert L.S == T + 5 and L.cells == (nf + 1) // 2 and L.Wt == L.Cw * L.S
        assert L.rows * L.Cw >= L.cells > (L.rows - 1) * L.Cw or L.cells == 0
        face, i, j, lower = tt.owners(L)
        assert face.shape == (L.Ht, L.Wt) and face.min(initial=0) >= -1 and face.max(initial=-1) < nf
        # every face owns texels of its own cell only, and every cell is split in two halves
        for f in range(nf):
            ys, xs = np.nonzero(face == f)
            k = f // 2
            assert len(xs) and (xs // L.S == k % L.Cw).all() and (ys // L.S == k // L.Cw).all()
            half = (T + 4) * (T + 5) // 2           # i + j <= T + 3: 1 + 2 + ... + (T + 4)
            assert len(xs) == (half if f % 2 == 0 else L.S * L.S - half)
            for x, y in tt.corner_texels(L, f):
                assert face[y, x] == f
        # the empty texels: the upper half of an odd nf's last cell and the trailing cells
        empty = face < 0
        cell = (np.arange(L.Ht)[:, None] // L.S) * L.Cw + np.arange(L.Wt)[None, :] // L.S
        assert np.array_equal(empty, (2 * cell + np.where(lower, 0, 1)) >= nf)
        # the default width is the smallest whose square holds the cells
        default = tt.Layout(nf, T)
        assert default.Cw >= 1 and default.Cw ** 2 >= default.cells
        assert default.Cw == 1 or (default.Cw - 1) ** 2 < default.cells


def _chart_points(rng, n=300):
    """Barycentrics (u, v): the corners, points on the three edges and random interior ones."""
    t = np.concatenate([np.linspace(0, 1, 23), rng.random(20)])
    edges = [np.stack([t, 0 * t], 1), np.stack([0 * t, t], 1), np.stack([t, 1 - t], 1)]
    inner = rng.random((n, 2))
    over = inner.sum(1) > 1
    inner[over] = 1 - inner[over]
    corners = np.array([[0, 0], [1, 0], [0, 1]], D)
    return np.concatenate([corners] + edges + [inner])


@pytest.mark.parametrize("nf,T", LAYOUTS)
def test_the_footprint_of_a_lookup_touches_only_the_faces_own_texels(nf, T):
    rng = np.random.default_rng(100 * nf + T)
    for L in _layouts(nf, T):
        face = tt.owners(L)[0]
        for f in range(nf):
            uv = _chart_points(rng)
            # (float32 barycentrics are what a render hands over; their sum may round above 1)
            for u, v in ((uv[:, 0], uv[:, 1]), (uv[:, 0].astype(F), uv[:, 1].astype(F))):
                keep = u.astype(D) + v.astype(D) <= 1
                u, v = u[keep], v[keep]
                x, y = tt.atlas_position(L, np.full(len(u), f), u, v)
                x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
                x1, y1 = np.minimum(x0 + 1, L.Wt - 1), np.minimum(y0 + 1, L.Ht - 1)
                fx, fy = x - x0, y - y0
                assert x0.min() >= 0 and y0.min() >= 0
                for tx, wx in ((x0, 1 - fx), (x1, fx)):
                    for ty, wy in ((y0, 1 - fy), (y1, fy)):
                        live = (wx != 0) & (wy != 0)
                        assert (face[ty[live], tx[live]] == f).all(), (L.Cw, f)
                xr, yr = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
                assert (face[yr, xr] == f).all(), (L.Cw, f)
            # the single-point helper agrees
            for u, v in ((0, 0), (1, 0), (0, 1), (0.25, 0.5)):
                for bilinear in (True, False):
                    assert all(face[ty, tx] == f for tx, ty in tt.footprint(L, f, u, v, bilinear))


@pytest.mark.parametrize("nf,T", LAYOUTS)
def test_the_packages_layout_and_uvs_are_the_restatements(nf, T):
    from raynet_amd import texture
    L = tt.Layout(nf, T)
    mine = texture.atlas_layout(nf, T)
    assert (mine.n_faces, mine.T, mine.S, mine.cells_per_row, mine.cells, mine.rows, mine.Wt,
            mine.Ht) == (nf, T, L.S, L.Cw, L.cells, L.rows, L.Wt, L.Ht)
    uvs = texture.face_uvs(nf, mine)
    assert uvs.shape == (nf, 3, 2) and uvs.dtype == D
    assert np.array_equal(uvs, tt.face_uvs(L))
    if nf:
        assert np.array_equal(texture.owned_texels(mine), tt.owners(L)[0] >= 0)
    # face_uvs lands on the corners: back to texel coordinates, whole numbers, owned by the face
    face = tt.owners(L)[0]
    for f in range(nf):
        x, y = uvs[f, :, 0] * L.Wt - 0.5, (1 - uvs[f, :, 1]) * L.Ht - 0.5
        assert np.abs(x - np.rint(x)).max() < 1e-9 and np.abs(y - np.rint(y)).max() < 1e-9
        assert np.array_equal(np.stack([np.rint(x), np.rint(y)], 1), tt.corner_texels(L, f))
        assert (face[np.rint(y).astype(int), np.rint(x).astype(int)] == f).all()


def test_the_packages_layout_refuses_what_the_entry_refuses():
    from raynet_amd import texture
    for bad in ((-1, 4), (4, 0), (4, 1025)):
        with pytest.raises(ValueError, match="atlas"):
            texture.atlas_layout(*bad)
    with pytest.raises(ValueError, match="cells_per_row"):
        texture.atlas_layout(4, 4, 0)
    with pytest.raises(ValueError, match="texels"):
        texture.atlas_layout(2 * 1000 * 1000, 16)
    big = texture.atlas_layout(1130000, 4)          # the unsimplified bench mesh fits at T = 4
    assert big.Wt <= 16384 and big.Ht <= 16384
    with pytest.raises(ValueError, match="faces"):
        texture.face_uvs(3, texture.atlas_layout(4, 2))


# ------------------------------------------------------------------------------ closed forms
def _quad(z=0.0, x0=-1.0, x1=1.0):
    """Two faces over the rectangle [x0, x1] x [-1, 1] at height z, counter-clockwise from above."""
    v = np.array([[x0, -1, z], [x1, -1, z], [x1, 1, z], [x0, 1, z]], F)
    return v, np.array([[0, 1, 2], [0, 2, 3]], I)


@pytest.mark.parametrize("T", [1, 4, 5])
@pytest.mark.parametrize("with_normals", [False, True])
def test_a_fronto_parallel_quad_under_an_affine_image(T, with_normals):
    cams, images, _ = at.plane_scene(centres=((0.05, 0.1),))
    vertices, faces = _quad()
    L = tt.Layout(2, T)
    normals = np.tile(np.array([[0, 0, 1]], F), (4, 1)) if with_normals else None
    texture, weight, views = tt.bake(vertices, faces, L, at.pack_cameras(cams), images,
                                     normals=normals)
    known, point, normal, u, v = tt.texel_points(vertices, faces, L, normals)
    assert known.all() and (views == 1).all() and (weight > 0).all()      # nf = 2 fills its cell
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1 + 1e-15).all()
    assert (normal[..., 2] > 0).all() and (normal[..., :2] == 0).all()
    # every owned texel, gutters included, has the analytic colour at its 3-D point
    want = at.affine_field(point[..., 0], point[..., 1])
    assert np.abs(texture.astype(D) - want).max() < 1e-6
    # a gutter texel's point lies on the rim of its face, an inner texel's is the chart's own
    face, i, j, lower = tt.owners(L)
    inner = lower & (i >= 1) & (j >= 1) & (i + j <= T + 2)
    assert np.array_equal(u[inner], (i[inner] - 1) / D(T))
    rim = lower & ~inner
    assert ((u[rim] == 0) | (v[rim] == 0) | (np.abs(u[rim] + v[rim] - 1) < 1e-15)).all()


@pytest.mark.parametrize("T", [4, 5])
def test_a_lookup_at_a_texels_own_barycentrics_returns_the_texel(T):
    rng = np.random.default_rng(T)
    nf = 5
    L = tt.Layout(nf, T)
    texture = rng.random((L.Ht, L.Wt, 3)).astype(F)
    face, i, j, lower = tt.owners(L)
    u = np.where(lower, (i - 1) / D(T), ((T + 3) - i) / D(T))
    v = np.where(lower, (j - 1) / D(T), ((T + 3) - j) / D(T))
    inside = (face >= 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    assert inside.sum() == nf * (T + 1) * (T + 2) // 2
    bary = np.stack([u[inside], v[inside]], 1).astype(F)
    for bilinear in (True, False):
        got = tt.sample(face[inside].astype(I), bary, L, texture, bilinear)
        assert np.abs(got.astype(D) - texture[inside]).max() < 1e-6
    # what is no lookup: 0
    f = np.array([-1, nf, 0, 0, 0, 0], I)
    b = np.array([[0.2, 0.2], [0.2, 0.2], [np.nan, 0.2], [0.2, -0.01], [1.01, 0], [0.2, 0.2]], F)
    got = tt.sample(f, b, L, texture)
    assert (got[:5] == 0).all() and (got[5] != 0).any()
    assert tt.sample(np.zeros((2, 3), I), np.zeros((2, 3, 2), F), L, texture).shape == (2, 3, 3)


def test_a_quad_behind_another_is_unseen_where_it_is_hidden():
    cams, images, plane_depths = at.plane_scene(centres=((0.05, 0.1),))
    cam, H, W = cams[0], 24, 32
    behind = -0.5
    front, front_faces = _quad(0.0, -1.0, 0.0)          # covers x <= 0 only
    rear, rear_faces = _quad(behind)
    vertices = np.concatenate([front, rear])
    faces = np.concatenate([front_faces, rear_faces + 4])
    # the depth map: the plane z = 0 where the pixel's ground point has x <= 0, else z = behind
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    gx, _ = cam.ground_point(X, Y)
    scale = (cam.height - behind) / cam.height
    depths = np.where(gx <= 0, plane_depths[0], plane_depths[0].astype(D) * scale).astype(F)[None]
    L = tt.Layout(4, 5)
    texture, weight, views = tt.bake(vertices, faces, L, at.pack_cameras(cams), images, depths,
                                     tol=0.05)
    known, point, _, _, _ = tt.texel_points(vertices, faces, L)
    face = tt.owners(L)[0]
    assert (views[face < 2] == 1).all()                 # the front quad is seen
    is_rear = face >= 2
    # where the rear point's pixel looks at the front quad (a pixel is 0.15 wide on the ground)
    shadow = (point[..., 0] - cam.cx) * cam.height / (cam.height - behind) + cam.cx
    hidden, clear = is_rear & (shadow < -0.15), is_rear & (shadow > 0.15)
    assert hidden.sum() > 20 and clear.sum() > 20
    assert (views[hidden] == 0).all() and (weight[hidden] == 0).all() and (texture[hidden] == 0).all()
    assert (views[clear] == 1).all()
    # without the depth map everything is seen
    assert (tt.bake(vertices, faces, L, at.pack_cameras(cams), images)[2] == 1).all()


def test_the_blend_against_the_best_of_two_views_of_different_obliquity():
    cams, images, _ = at.plane_scene(centres=((0.0, 0.0), (1.2, 0.0)), C=1)
    images = np.stack([np.full_like(images[0], 0.2), np.full_like(images[1], 0.8)])
    vertices, faces = _quad(0.0, -0.5, 0.5)
    L = tt.Layout(2, 3)
    rows = at.pack_cameras(cams)
    blend, w0, views0 = tt.bake(vertices, faces, L, rows, images, mode=0)
    best, w1, views1 = tt.bake(vertices, faces, L, rows, images, mode=1)
    assert (views0 == 3).all() and np.array_equal(views0, views1) and np.array_equal(w0, w1)
    point = tt.texel_points(vertices, faces, L)[1]
    # cos^2 = height^2 / dd: the view straight above faces every texel better
    cos2 = [cams[k].height ** 2 / ((point[..., 0] - cams[k].cx) ** 2 +
                                   (point[..., 1] - cams[k].cy) ** 2 + cams[k].height ** 2)
            for k in range(2)]
    assert (cos2[0] > cos2[1]).all()
    assert (best[..., 0] == F(0.2)).all()
    assert ((blend[..., 0] > F(0.2)) & (blend[..., 0] < F(0.5))).all()
    # the other way round: the oblique view first changes the mask's bits, not the colours
    swapped = tt.bake(vertices, faces, L, rows[::-1], images[::-1], mode=1)
    assert (swapped[0][..., 0] == F(0.2)).all()
    # one view only: blend and best agree to the bit
    one0 = tt.bake(vertices, faces, L, rows[:1], images[:1], mode=0)[0]
    one1 = tt.bake(vertices, faces, L, rows[:1], images[:1], mode=1)[0]
    assert (one1 == F(0.2)).all() and np.abs(one0 - one1).max() <= np.spacing(F(0.2))


@pytest.mark.parametrize("mode", [0, 1])
def test_the_corner_texels_of_a_bake_are_the_colours_of_the_vertices(mode):
    """At a chart's corner (u, v) is (0, 0), (1, 0) or (0, 1): the texel's point and normal are
    the vertex's own, so the bake there and project_colors at the vertex are the same bits."""
    s = tt.corner_scene()
    views = (s["cameras"], s["images"], s["depths"], s["tol"], s["min_cos"], s["border"], mode)
    known, point, normal, u, v = tt.texel_points(s["vertices"], s["faces"], s["L"], s["normals"])
    order = s["faces"].reshape(-1)
    p, n, cu, cv = tt.corners_of(s, (point, normal, u, v))
    assert np.array_equal(p, s["vertices"][order].astype(D))
    assert np.array_equal(n, s["normals"][order].astype(D))
    assert np.array_equal(np.stack([cu, cv], 1), np.tile([[0, 0], [1, 0], [0, 1]], (2, 1)))
    baked = tt.corners_of(s, tt.bake(s["vertices"], s["faces"], s["L"], s["cameras"], s["images"],
                                     s["depths"], s["normals"], s["tol"], s["min_cos"], s["border"],
                                     mode))
    colors, weight, seen = at.project_colors(s["vertices"], s["normals"], *views)
    assert np.array_equal(baked[0].view(I), colors[order].view(I))
    assert np.array_equal(baked[1].view(I), weight[order].view(I))
    assert np.array_equal(baked[2], seen[order]) and baked[2].dtype == np.uint32
    # the comparison is not one of zeros: every corner is seen, one by two views of different
    # weights, where the blend and the best view differ
    assert (seen != 0).all()
    single = [at.project_colors(s["vertices"], s["normals"], s["cameras"][k:k + 1],
                                s["images"][k:k + 1], s["depths"][k:k + 1], *views[3:])[1]
              for k in range(3)]
    two = [i for i in range(4) if ((seen[i] & 3) == 3 and single[0][i] != single[1][i])]
    assert two
    other = at.project_colors(s["vertices"], s["normals"], *views[:-1], 1 - mode)[0]
    assert not np.array_equal(other[two], colors[two])
