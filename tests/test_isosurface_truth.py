"""tests/isosurface_truth.py held to properties nobody has to trust: the surface of marching
tetrahedra over the Kuhn split is a closed, consistently oriented 2-manifold of the right genus
and volume, for smooth inputs, for inputs cut by the border, and for values equal to the iso
value.  No GPU."""
import numpy as np

import isosurface_truth as it

F = np.float32


def _extract(belief, iso=0.5, closed=True):
    bbox, axes = it.unit_frame(belief.shape)
    return it.extract(belief, iso, closed, axes, bbox)


def _assert_closed_and_oriented(v, f):
    E, two, repeated, _ = it.edge_census(f)
    assert len(f) > 0
    assert E == two, "%d of %d edges are not in exactly two faces" % (E - two, E)
    assert repeated == 0, "%d directed edges are used more than once" % repeated
    assert 3 * len(f) == 2 * E                     # hence every directed edge exactly once
    assert len(np.unique(f.ravel())) == len(v), "unused vertices"


def test_the_table_has_a_closed_case_structure():
    for ti, tet in enumerate(it.TETS):
        for case in range(16):
            tris = it.TABLE[ti][case]
            inside = bin(case).count("1")
            assert len(tris) == min(inside, 4 - inside)
            for tri in tris:
                for lo, d in tri:
                    assert lo in tet and (lo | d) in tet and lo & d == 0 and 1 <= d <= 7
            # a case and its complement: the same triangles, turned round
            other = it.TABLE[ti][15 - case]
            assert sorted(sorted(t) for t in tris) == sorted(sorted(t) for t in other)


def test_logistic_ball():
    v, f = _extract(it.logistic_ball())
    _assert_closed_and_oriented(v, f)
    assert it.euler_characteristic(v, f) == 2
    volume = it.signed_volume(v, f)
    want = 4.0 / 3.0 * np.pi * 3.7 ** 3
    print("logistic ball: %d vertices, %d faces, signed volume %.4f (sphere %.4f, %+.2f %%)"
          % (len(v), len(f), volume, want, 100 * (volume / want - 1)))
    assert volume > 0 and abs(volume / want - 1) <= 0.05
    assert v.dtype == F and f.dtype == np.int32


def test_ball_cut_by_the_border_is_closed_by_the_padding():
    belief = it.cut_ball()
    assert (belief[0] >= 0.5).any()
    v, f = _extract(belief)
    _assert_closed_and_oriented(v, f)
    assert it.euler_characteristic(v, f) == 2
    assert it.signed_volume(v, f) > 0
    assert v[:, 0].min() < 0                       # vertices on the edges into the padding


def test_torus():
    v, f = _extract(it.torus())
    _assert_closed_and_oriented(v, f)
    assert it.euler_characteristic(v, f) == 0
    assert it.signed_volume(v, f) > 0


def test_noise_with_values_equal_to_the_iso_value():
    belief = it.noise()
    assert (belief == F(0.5)).sum() >= 20
    v, f = _extract(belief)
    _assert_closed_and_oriented(v, f)
    assert it.signed_volume(v, f) > 0
    # such vertices sit on lattice points, and some triangles have no area
    tri = v[f.astype(np.int64)].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).any() and (area > 0).any()


def test_open_extraction_is_oriented_and_open_only_on_the_hull():
    grid = (7, 6, 5)
    belief = np.random.default_rng(8).uniform(0.05, 0.95, grid).astype(F)
    v, f = _extract(belief, closed=False)
    E, two, repeated, boundary = it.edge_census(f)
    assert repeated == 0 and len(boundary) > 0 and E == two + len(boundary)
    # both ends of a boundary edge lie on one face of the lattice's hull
    hi = np.array(grid, np.float64) - 1
    a, b = v[boundary[:, 0]].astype(np.float64), v[boundary[:, 1]].astype(np.float64)
    on_face = ((a == 0) & (b == 0)) | ((a == hi) & (b == hi))
    assert on_face.any(axis=1).all()
    # and the closed extraction of the same grid is closed
    _assert_closed_and_oriented(*_extract(belief))


def test_planted_voxel_has_the_closed_form():
    where = (1, 2, 1)
    belief = it.planted_voxel(where=where)
    bbox = np.array([-0.8, -0.6, -0.4, 0.8, 0.65, 0.41], F)
    grid = belief.shape
    axes = [(F(bbox[a]) + np.arange(grid[a], dtype=F) * F(0.4) + F(0.2)).astype(F) for a in range(3)]
    v, f = it.extract(belief, 0.5, True, axes, bbox)
    _assert_closed_and_oriented(v, f)
    assert it.euler_characteristic(v, f) == 2
    # 14 edges leave a lattice point along the Kuhn directions: 7 from it, 7 into it
    assert len(v) == 14 and len(f) == 24
    t_out = F(F(F(0.5) - F(0.9)) / F(F(0) - F(0.9)))          # from the voxel to a neighbour
    t_in = F(F(F(0.5) - F(0)) / F(F(0.9) - F(0)))             # from a neighbour to the voxel
    A = [it.padded_axis(axes[a], bbox[a], bbox[3 + a], grid[a], True) for a in range(3)]
    p = [w + 1 for w in where]                                 # the voxel as a lattice point
    want = []
    for d in range(1, 8):                                      # edges (p - d, d): they come first
        o = [(d >> a) & 1 for a in range(3)]
        want.append(((p[0] - o[0], p[1] - o[1], p[2] - o[2]), d,
                     [F(A[a][p[a] - 1] + F(t_in * F(A[a][p[a]] - A[a][p[a] - 1]))) if o[a]
                      else A[a][p[a]] for a in range(3)]))
    for d in range(1, 8):
        o = [(d >> a) & 1 for a in range(3)]
        want.append((tuple(p), d,
                     [F(A[a][p[a]] + F(t_out * F(A[a][p[a] + 1] - A[a][p[a]]))) if o[a]
                      else A[a][p[a]] for a in range(3)]))
    n = [s + 2 for s in grid]
    want.sort(key=lambda w: ((w[0][0] * n[1] + w[0][1]) * n[2] + w[0][2], w[1]))
    got = v.view(np.int32)
    exp = np.array([w[2] for w in want], F).view(np.int32)
    assert np.array_equal(got, exp)


def test_empty_meshes():
    for belief, closed in [(np.full((4, 5, 6), 0.2, F), True), (np.full((4, 5, 6), 0.2, F), False),
                           (np.full((4, 5, 6), 0.9, F), False),
                           (it.logistic_ball((1, 11, 10), (0, 5, 5)), False),
                           (it.logistic_ball((12, 1, 10), (5, 0, 5)), False),
                           (it.logistic_ball((12, 11, 1), (5, 5, 0)), False)]:
        v, f = _extract(belief, closed=closed)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == F and f.dtype == np.int32


def test_all_above_is_a_closed_box():
    v, f = _extract(np.full((3, 4, 5), 0.9, F))
    _assert_closed_and_oriented(v, f)
    assert it.euler_characteristic(v, f) == 2
    # iso at 5/9 of the way out of every border voxel
    t = 1 - 0.5 / 0.9
    want = (2 + 2 * t) * (3 + 2 * t) * (4 + 2 * t)
    assert 0 < it.signed_volume(v, f) <= want and it.signed_volume(v, f) > 0.9 * want


def test_one_voxel_grid():
    v, f = _extract(np.full((1, 1, 1), 0.9, F))
    _assert_closed_and_oriented(v, f)
    assert len(v) == 14 and len(f) == 24 and it.euler_characteristic(v, f) == 2
