"""tests/render_truth.py, the NumPy restatement of rn_mesh_render, without
a GPU: on the rays of the reference's golden it finds what tests/raycast_truth.py finds (which
tests/test_raycast_reference.py pins to the reference bit for bit), and on meshes small enough to
reason about it gives what the definition says: the barycentrics and colours at a triangle's
corners, zeros on a miss, the lower face of a coincident pair, a constant colour, unit normals."""
import os

import numpy as np

import raycast_truth as rt
import render_truth as rd
from conftest import GOLDEN

F = np.float32
D = np.float64


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_faces_points_and_depths_are_the_pinned_restatements_on_the_golden_rays():
    g = np.load(os.path.join(GOLDEN, "ref_raycast.npz"))
    tri = g["ref_triangles"]
    cases = [(g["pix_o"][c], g["pix_d"][c]) for c in range(len(g["K"]))] + [(g["ray_o"], g["ray_d"])]
    hits = 0
    for o, d in cases:
        want_points, want_face = rt.first_hits(o, d, tri)
        face, depth, bary, points, _ = rd.cast(o, d, tri, o[0])
        assert np.array_equal(face, want_face)
        assert np.array_equal(_bits(points), _bits(want_points))
        want_depth = rt.depths(want_points, want_face, o[0])
        assert np.array_equal(_bits(depth[face >= 0]), _bits(want_depth[face >= 0].astype(F)))
        assert (depth[face < 0] == 0).all() and (bary[face < 0] == 0).all()
        # the barycentrics name the hit: (1 - u - v) p0 + u p1 + v p2, up to fp32 rounding
        t = tri[face[face >= 0]].astype(D).reshape(-1, 3, 3)
        u, v = bary[face >= 0, 0:1].astype(D), bary[face >= 0, 1:2].astype(D)
        at = (1 - u - v) * t[:, 0] + u * t[:, 1] + v * t[:, 2]
        scale = np.abs(tri).max()
        assert np.abs(at - points[face >= 0]).max() <= 1e-4 * scale
        hits += int((face >= 0).sum())
    assert hits > 2000


def test_one_triangle_its_corners_and_the_misses():
    vertices, faces, corners = rd.one_triangle()
    colors = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]], F)
    normals = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1]], F)
    got = rd.render(vertices, faces, rd.axis_camera(8), 8, 8, colors, normals)
    for (x, y), want, k in zip(corners, [(0, 0), (1, 0), (0, 1)], range(3)):
        assert got.face[0, y, x] == 0, (x, y)
        assert np.abs(got.bary[0, y, x] - want).max() <= 4e-6, (x, y, got.bary[0, y, x])
        assert np.abs(got.color[0, y, x].astype(D) - colors[k]).max() <= 1e-6, (x, y)
    hit = got.face[0] == 0
    # the pixels inside: x, y >= 2 and x + y <= 8
    ys, xs = np.mgrid[0:8, 0:8]
    assert np.array_equal(hit, (xs >= 2) & (ys >= 2) & (xs + ys <= 8))
    miss = ~hit
    assert (got.face[0][miss] == -1).all() and (_bits(got.depth[0][miss]) == 0).all()
    assert (_bits(got.bary[0][miss]) == 0).all() and (_bits(got.color[0][miss]) == 0).all()
    assert (_bits(got.normal[0][miss]) == 0).all()
    # the depth of the hit straight ahead: pixel (4, 4) looks along +z at the plane z = 4
    assert got.depth[0, 4, 4] == 4 and not got.ties.any()


def test_of_two_coincident_triangles_the_lower_index_wins():
    vertices, faces = rd.coincident_pair()
    colors = np.repeat(np.array([[0.25], [0.75]], F), 3, axis=0)
    got = rd.render(vertices, faces, rd.axis_camera(8), 8, 8, colors)
    hit = got.face[0] >= 0
    assert hit.sum() == 15 and (got.face[0][hit] == 0).all() and got.ties[0][hit].all()
    assert np.abs(got.color[0][hit] - 0.25).max() <= 1e-7
    swapped = rd.render(vertices, faces[::-1], rd.axis_camera(8), 8, 8, colors)
    assert (swapped.face[0][hit] == 0).all() and np.abs(swapped.color[0][hit] - 0.75).max() <= 1e-7


def test_the_shared_edge_of_a_square_belongs_to_one_face_per_pixel():
    vertices, faces = rd.square()
    got = rd.render(vertices, faces, rd.axis_camera(8), 8, 8)
    ys, xs = np.mgrid[0:8, 0:8]
    inside = (xs >= 1) & (xs <= 7) & (ys >= 1) & (ys <= 7)
    edge = xs == ys
    # (a ray on the edge itself has u == 0 in one face and v == 0 in the other up to rounding:
    # either face, or neither, is what the definition gives; the kernel must give the same)
    assert np.array_equal((got.face[0] >= 0) & ~edge, inside & ~edge) and (got.face[0][~inside] == -1).all()
    assert (got.face[0][inside & (xs > ys)] == 0).all() and (got.face[0][inside & (xs < ys)] == 1).all()
    assert (got.depth[0][got.face[0] >= 0] >= 4).all()
    print("faces along the shared edge:", got.face[0][edge & inside].tolist())


def test_a_constant_colour_renders_as_that_colour_within_one_ulp():
    vertices, faces = rd.icosphere(2)
    rows = rd.ring_rows(3, 20, 30)
    for value in (F(1.0), F(0.1), F(1 / 3), F(200 / 255)):
        colors = np.full((len(vertices), 3), value, F)
        got = rd.render(vertices, faces, rows, 20, 30, colors)
        hit = got.face >= 0
        assert hit.sum() > 200
        ulps = np.abs(_bits(got.color[hit]).astype(np.int64) - int(_bits(value).reshape(-1)[0]))
        assert ulps.max() <= 1, (value, ulps.max())
        assert (_bits(got.color[~hit]) == 0).all()


def test_interpolated_normals_are_unit_or_exactly_zero():
    vertices, faces = rd.icosphere(2)
    rows = rd.ring_rows(3, 20, 30)
    normals = rd.vertex_attributes(len(vertices), 3, seed=3)[1]
    normals[faces[5]] = 0                              # a face without normals
    normals[faces[40, 0]] = -normals[faces[40, 1]]     # and vertices whose normals oppose
    got = rd.render(vertices, faces, rows, 20, 30, normals=normals)
    length = np.sqrt((got.normal.astype(D) ** 2).sum(-1))
    zero = (_bits(got.normal) == 0).all(-1)
    assert np.abs(length[~zero] - 1).max() <= 1e-6
    assert zero[got.face < 0].all() and (~zero).sum() > 200
    # the sphere's own normals come out as the hit's direction from its centre
    own = (vertices / np.linalg.norm(vertices, axis=1)[:, None]).astype(F)
    got = rd.render(vertices, faces, rows[:1], 20, 30, normals=own)
    hit = got.face[0] >= 0
    o, dst = rd.view_rays(rows[0], 20, 30)
    _, _, _, points, _ = rd.cast(o, dst, vertices[faces].reshape(-1, 9), rows[0, 12:])
    radial = points / np.linalg.norm(points, axis=1)[:, None].clip(1e-30)
    assert np.abs(got.normal[0][hit] - radial.reshape(20, 30, 3)[hit]).max() <= 5e-3
