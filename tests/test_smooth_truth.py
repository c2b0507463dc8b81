"""The restatement of the smoothing (tests/smooth_truth.py) held to properties nobody has to trust
(no GPU, no library): the side-by-side step against the definition line by line, what must not
move, a plane that stays a plane, the clamp, where a NaN gets to, and on the terraced iso-surface
of a binary ball that the normals get better and that lambda | mu keeps the volume where plain
Laplacian smoothing loses it."""
import numpy as np
import pytest

import appearance_truth as at
import components_truth as ct
import isosurface_truth as it
import smooth_truth as st

F = np.float32
D = np.float64


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def ball():
    vertices, faces = st.binary_ball()
    assert vertices.shape == (2908, 3) and faces.shape == (5812, 3)
    assert it.is_closed_and_oriented(vertices, faces)
    return vertices, faces


def test_the_side_by_side_step_is_the_definition_line_by_line():
    cases = [st.strip(67, 1), st.strip(67, 2, permuted=True), st.star(40, 3), st.star(40, 4, True),
             st.flat_patch(5)]
    for vertices, faces in cases:
        nv = len(vertices)
        fixed = st.boundary_vertices(faces, nv)
        for kw in (dict(iterations=2), dict(iterations=1, mu=0.0, max_move=0.05),
                   dict(iterations=3, fixed=fixed), dict(iterations=1, lam=1.0, mu=-1.0)):
            a = st.smooth(vertices, faces, **kw)
            b = st.smooth(vertices, faces, one_step=st.step_plain, **kw)
            assert np.array_equal(_bits(a), _bits(b)), kw
    # garbage in all three index arrays, reversed and overhanging ranges
    vertices, faces = st.strip(40, 5, permuted=True)
    offsets, corners = at.corner_table(faces, 40)
    bad_faces, _ = st.with_bad_faces(faces, 40, seed=6, fraction=0.2)
    bad_corners, _ = st.with_bad_corners(corners, len(faces), seed=7, fraction=0.2)
    bad_offsets = offsets.copy()
    bad_offsets[[3, 9, 20, 31]] = [-5, 10 ** 6, 2, -2 ** 31]
    a = st.smooth(vertices, bad_faces, 2, offsets=bad_offsets, corners=bad_corners)
    b = st.smooth(vertices, bad_faces, 2, offsets=bad_offsets, corners=bad_corners,
                  one_step=st.step_plain)
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a), _bits(vertices))


def test_the_ring_names_the_two_other_vertices_in_the_faces_order():
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    offsets, corners = at.corner_table(faces, 4)
    assert corners.tolist() == [0, 1, 4, 2, 3, 5] and offsets.tolist() == [0, 1, 3, 5, 6]
    assert st.ring_of(faces, 4, corners).tolist() == [[1, 2], [2, 0], [3, 2], [0, 1], [1, 3], [2, 1]]
    # a corner outside the table, a face with an index outside the vertices
    assert st.ring_of(faces, 4, [6, -1, 0, 1, 2, 2 ** 31 - 1]).tolist() == \
        [[-1, -1], [-1, -1], [1, 2], [2, 0], [0, 1], [-1, -1]]
    assert st.ring_of(faces, 3, corners).tolist() == [[1, 2], [2, 0]] + [[-1, -1]] * 1 + [[0, 1]] + \
        [[-1, -1]] * 2


def test_no_iteration_no_face_and_a_pin_keep_the_bits():
    vertices, faces = st.strip(50, 8, permuted=True)
    vertices[7] = [-0.0, 1e-42, 3.0]                        # a signed zero and a denormal
    assert np.array_equal(_bits(st.smooth(vertices, faces, 0)), _bits(vertices))
    fixed = np.zeros(50, np.uint8)
    fixed[[0, 7, 20, 49]] = [1, 255, 2, 1]
    out = st.smooth(vertices, faces, 4, fixed=fixed)
    assert np.array_equal(_bits(out[fixed != 0]), _bits(vertices[fixed != 0]))
    assert (_bits(out[fixed == 0]) != _bits(vertices[fixed == 0])).any(1).all()
    # vertices in no face, in between and at the end
    loose = np.concatenate([vertices, st.positions(6, 9)])
    out = st.smooth(loose, faces, 3)
    assert np.array_equal(_bits(out[50:]), _bits(loose[50:])) and not np.array_equal(out[:50], loose[:50])
    none = st.smooth(loose, np.zeros((0, 3), np.int32), 3)
    assert np.array_equal(_bits(none), _bits(loose))


def test_coinciding_vertices_stay_put():
    _, faces = st.strip(30, 0)
    for point in ([0.1, -2.7, 1e6], [1e-30, 3.3, -0.7]):
        vertices = np.tile(np.array(point, F), (30, 1))
        for kw in (dict(), dict(mu=0.0), dict(lam=1.0, mu=-1.0)):
            assert np.array_equal(_bits(st.smooth(vertices, faces, 5, **kw)), _bits(vertices)), kw


def test_a_flat_patch_with_its_border_pinned_stays_in_its_plane():
    vertices, faces = st.flat_patch(9)
    border = st.boundary_vertices(faces, len(vertices))
    assert border.sum() == 4 * 8
    # (the interior is regular, so x and y stay too where every neighbour is inside the patch;
    # the plane is what is exact for every vertex: sums of 1.25 are exact, and their mean is 1.25)
    out = st.smooth(vertices, faces, 10, fixed=border)
    assert np.array_equal(_bits(out[:, 2]), _bits(vertices[:, 2]))
    assert np.array_equal(_bits(out[border]), _bits(vertices[border]))
    # shake the interior within the plane: it moves, and stays in the plane
    rng = np.random.default_rng(3)
    shaken = vertices.copy()
    shaken[~border, :2] += (0.25 * rng.integers(-1, 2, size=((~border).sum(), 2))).astype(F)
    out = st.smooth(shaken, faces, 10, fixed=border)
    assert np.array_equal(_bits(out[:, 2]), _bits(shaken[:, 2]))
    assert not np.array_equal(out[~border, :2], shaken[~border, :2])


def test_the_clamp_holds_in_every_coordinate_and_is_met(ball):
    vertices, faces = ball
    for d in (0.05, 0.25):
        out = st.smooth(vertices, faces, 10, mu=0.0, max_move=d)
        # x is clamped in fp64 to [in - d, in + d] and rounded to f32 once, and rounding is
        # monotone: the f32 result lies between the two bounds rounded to f32, exactly.  (That is
        # |out - in| <= d up to half an f32 ulp of the coordinate, and no more can be asked: the
        # bound itself need not be an f32.)
        lo, hi = st.clamp_bounds(vertices, d)
        assert (out >= lo).all() and (out <= hi).all()
        assert ((out == lo) | (out == hi)).any(), "the clamp was never met"
        moved = np.abs(out.astype(D) - vertices.astype(D))
        assert moved.max() <= d + 0.5 * float(np.spacing(np.abs(out).max()))
    free = np.abs(st.smooth(vertices, faces, 10, mu=0.0).astype(D) - vertices.astype(D))
    assert free.max() > 0.25


def test_a_nan_reaches_exactly_the_vertices_that_share_a_face_with_it(ball):
    vertices, faces = ball
    for planted, value in ((17, np.nan), (1500, np.inf)):
        v = vertices.copy()
        v[planted, 1] = value
        out = st.smooth(v, faces, 1, mu=0.0)
        near = np.zeros(len(v), bool)
        near[faces[(faces == planted).any(1)].reshape(-1)] = True
        bad = ~np.isfinite(out).all(1)
        # the vertex itself: its neighbours' mean is finite, p + t (mean - p) is not
        assert near[planted] and np.array_equal(bad, near)
        assert np.isfinite(out[:, [0, 2]]).all()            # and only that coordinate


def test_on_the_binary_ball_the_normals_improve_and_taubin_keeps_the_volume(ball):
    vertices, faces = ball
    taubin = st.smooth(vertices, faces, 10, 0.5, -0.53)
    laplace = st.smooth(vertices, faces, 10, 0.5, 0.0)
    rows = []
    for name, v in (("unsmoothed", vertices), ("taubin", taubin), ("laplace", laplace)):
        rows.append((name, st.mean_angle_to_radial(v, faces, st.BALL_CENTRE),
                     st.mean_radial_error(v, st.BALL_CENTRE, st.BALL_RADIUS),
                     it.signed_volume(v, faces),
                     float(np.abs(v.astype(D) - vertices.astype(D)).max())))
        print("%-10s angle %.1f deg, |r - R| %.3f, volume %.1f, farthest move %.2f" % rows[-1])
    (_, a0, _, vol0, _), (_, a1, _, vol1, _), (_, a2, _, vol2, _) = rows
    assert a1 < a0 and a2 < a0
    assert abs(vol1 - vol0) < abs(vol2 - vol0)


def test_the_border_by_the_dictionary():
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    assert st.boundary_vertices(faces, 5).tolist() == [True, True, True, True, False]
    tet, nv = ct.tetrahedra(2)
    assert not st.boundary_vertices(tet, nv).any()
    assert st.boundary_vertices(tet[1:], nv).tolist() == [True, True, True, False] + [False] * 4
    # a degenerate face (a, a, b) has the edge (a, b) twice; a face with an index outside has none
    assert not st.boundary_vertices(np.array([[1, 1, 3], [0, 2, 9]], np.int32), 5).any()
    assert st.boundary_vertices(np.array([[1, 1, 3], [0, 2, 4]], np.int32), 5).tolist() == \
        [True, False, True, False, True]
