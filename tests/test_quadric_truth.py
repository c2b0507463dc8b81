"""The restatement of rn_mesh_place_quadric (tests/quadric_truth.py) held to what the placement is
for (no GPU): on the rotated cube the placed vertices lie closer to the surface than the means and
none lies farther; a flat region keeps its bits; the order of the faces plays no part; the sums
stay within the bound the header states; clusters nothing constrains fall back; the regulariser
and the clamp do what they say."""
import numpy as np

import quadric_truth as qt
import simplify_truth as sp

F = np.float32
D = np.float64
I = np.int32
CELL = 0.4


def _cube():
    vertices, faces = qt.rotated_cube(6)
    assert vertices.shape == (218, 3) and faces.shape == (432, 3)
    mean, out, counts, grid = qt.simplify_and_place(vertices, faces, CELL)
    assert len(mean[0]) == 48
    return vertices, faces, mean, out, counts, grid


def test_on_the_rotated_cube_the_placed_vertices_are_closer_and_none_is_farther():
    """The issue's relation: the RMS distance to the cube's surface under quadric placement is
    strictly below that under the mean, and no vertex is farther than under the mean by more than
    1e-6 of a cell.  Both values are printed (DESIGN.md section 28 quotes them)."""
    vertices, faces, mean, out, counts, grid = _cube()
    at_mean, at_quadric = qt.cube_distance(mean[0]) / CELL, qt.cube_distance(out) / CELL
    rms = [float(np.sqrt((d ** 2).mean())) for d in (at_mean, at_quadric)]
    print("rotated cube, 6 x 6 quads, cell 0.4, 48 clusters, in cell sides: mean placement RMS "
          "%.3e (max %.3e), quadric placement RMS %.3e (max %.3e); %d moved, %d fell back"
          % (rms[0], at_mean.max(), rms[1], at_quadric.max(), counts[0], counts[1]))
    assert rms[1] < rms[0]
    assert (at_quadric <= at_mean + 1e-6).all()
    assert counts[1] == 0 and 0 < counts[0] <= 48
    assert out.dtype == F and out.shape == mean[0].shape


def test_a_flat_region_keeps_the_bits_of_the_means():
    """Every face lies in z = 0.25, which is a float and a double: n = (0, 0, +-1), r_z = 0 and d
    = 0 exactly, so x = 0 and every output is its mean's bits -- and not through the fallback."""
    vertices, faces = qt.flat_square()
    mean, out, counts, grid = qt.simplify_and_place(vertices, faces, 1.0)
    assert len(mean[0]) > 4 and (mean[0][:, 2] == F(0.25)).all()
    S = qt.sums(vertices, faces, mean[3], mean[0], grid[1])
    assert (S[:, 6:9] == 0).all() and (S[:, 9] > 0).all() and (S[:, 10] > 1).sum() > 4
    assert np.array_equal(qt.bits(out), qt.bits(mean[0]))
    assert counts.tolist() == [0, 0]


def test_the_order_of_the_faces_plays_no_part_and_the_loop_is_the_vectorised_form():
    """Integer sums: the faces as rows of the array in any order, and the loop of the definition
    over them in any order, give the same eleven words and the same bits.  The corners of a face
    turned (b, c, a) name the same plane through another base corner: the roundings of N differ
    in the last place, so the sums may differ by a few units of 2^-30 and the positions by far
    less than the 1e-6 of a cell the quality relation allows -- held to that, not to the bit."""
    vertices, faces, mean, out, counts, grid = _cube()
    rng = np.random.default_rng(5)
    shuffled = rng.permutation(len(faces))
    got = qt.place(vertices, faces[shuffled], mean[3], mean[0], grid[1])
    assert np.array_equal(qt.bits(got[0]), qt.bits(out)) and np.array_equal(got[1], counts)
    S = qt.sums(vertices, faces, mean[3], mean[0], grid[1])
    for order in (None, shuffled, np.arange(len(faces))[::-1]):
        plain = qt.place_plain(vertices, faces, mean[3], mean[0], grid[1], order=order)
        assert np.array_equal(plain[2], S)
        assert np.array_equal(qt.bits(plain[0]), qt.bits(out)) and np.array_equal(plain[1], counts)
    turned = qt.place(vertices, faces[:, [1, 2, 0]], mean[3], mean[0], grid[1])
    assert np.abs(turned[0].astype(D) - out.astype(D)).max() < 1e-6 * CELL
    flipped = qt.place(vertices, faces[:, ::-1], mean[3], mean[0], grid[1])     # n -> -n, d -> -d
    assert np.abs(flipped[0].astype(D) - out.astype(D)).max() < 1e-6 * CELL


def test_five_thousand_faces_of_weight_one_in_one_cluster_stay_within_the_bound():
    """The header's bound: every term below 3.47 in magnitude, so every integer below 2^32, and a
    sum of nf of them below nf 2^32 -- 2^62 at the 2^30 faces an entry takes.  Large faces (weight
    1) whose corners lie at the far ends of the reach."""
    rng = np.random.default_rng(7)
    nf = 5000
    corners = rng.uniform(-1.9, 1.9, (nf, 3, 3))
    vertices = corners.reshape(-1, 3).astype(F)
    faces = np.arange(3 * nf, dtype=I).reshape(nf, 3)
    cluster = np.zeros(3 * nf, I)
    positions = np.zeros((1, 3), F)
    S = qt.sums(vertices, faces, cluster, positions, 1.0)
    assert S[0, 10] == 3 * nf
    assert S[0, 9] > 0.9 * nf * 2 ** 30                 # nearly every face weighs 1
    assert (np.abs(S[0, :10]) <= nf * int(qt.TERM_BOUND * 2 ** 30)).all()
    assert nf * int(qt.TERM_BOUND * 2 ** 30) * (2 ** 30 // nf) < 2 ** 62
    assert S[0, 0] + S[0, 3] + S[0, 5] <= S[0, 9] + 3 * nf      # the trace of n n^T is 1
    out, counts = qt.place(vertices, faces, cluster, positions, 1.0)
    assert np.isfinite(out).all() and counts.tolist() == [1, 0]


def test_clusters_without_a_plane_or_with_one_member_fall_back():
    # four vertices on a line in one cell, two far ones: every face in the cluster has no area
    vertices = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3], [0.4, 0.4, 0.4],
                         [5.5, 0.5, 0.5], [0.5, 5.5, 0.5]], F)
    faces = np.array([[0, 1, 2], [1, 2, 3], [0, 2, 3], [0, 4, 5]], I)
    faces[3] = [0, 0, 4]                                # no area either, but it names two clusters
    cluster = np.array([0, 0, 0, 0, 1, 2], I)
    positions = np.array([[0.25, 0.25, 0.25], [5.5, 0.5, 0.5], [0.5, 5.5, 0.5]], F)
    S = qt.sums(vertices, faces, cluster, positions, 1.0)
    assert S[:, 10].tolist() == [4, 1, 1] and (S[:, :10] == 0).all()
    out, counts = qt.place(vertices, faces, cluster, positions, 1.0)
    assert np.array_equal(qt.bits(out), qt.bits(positions))
    assert counts.tolist() == [0, 1]                    # the cluster of four was refused
    # a real face between three clusters of one member each: sums, but nothing moves
    faces = np.array([[0, 4, 5]], I)
    cluster = np.array([0, -1, -1, -1, 1, 2], I)
    positions = np.array([[0.1, 0.1, 0.6], [5.5, 0.5, 0.5], [0.5, 5.5, 0.5]], F)
    S = qt.sums(vertices, faces, cluster, positions, 1.0)
    assert S[:, 10].tolist() == [1, 1, 1] and (S[:, 9] > 0).all() and S[0, 8] != 0
    out, counts = qt.place(vertices, faces, cluster, positions, 1.0)
    assert np.array_equal(qt.bits(out), qt.bits(positions)) and counts.tolist() == [0, 0]
    # a NaN position keeps its payload
    positions = positions.copy()
    positions.view(np.uint32)[0, 1] = 0x7FC12345
    out, _ = qt.place(vertices, faces, np.array([0, 0, -1, -1, 1, 2], I), positions, 1.0)
    assert np.array_equal(qt.bits(out), qt.bits(positions))


def test_the_regulariser_holds_vertices_back_and_max_move_clamps_them():
    vertices, faces, mean, out, counts, grid = _cube()
    move = np.abs(out.astype(D) - mean[0].astype(D)).max(1)
    held, _ = qt.place(vertices, faces, mean[3], mean[0], grid[1], regularization=1.0)
    held_move = np.abs(held.astype(D) - mean[0].astype(D)).max(1)
    moved = move > 0
    assert moved.sum() > 8 and (held_move[moved] < move[moved]).all()
    assert np.linalg.norm(held.astype(D) - mean[0]) < np.linalg.norm(out.astype(D) - mean[0])
    # the clusters at the cube's corners move farthest: more than 0.05 of a cell, so 0.05 clamps them
    limit = 0.05
    assert move.max() > limit * CELL
    clamped, n = qt.place(vertices, faces, mean[3], mean[0], grid[1], max_move=limit)
    clamped_move = np.abs(clamped.astype(D) - mean[0].astype(D))
    slack = np.abs(mean[0].astype(D)).max() * 2.0 ** -23         # the rounding to float32
    assert clamped_move.max() <= limit * CELL + slack
    assert clamped_move.max() >= limit * CELL - slack
    far = move > limit * CELL + slack
    assert far.any() and not np.array_equal(qt.bits(clamped[far]), qt.bits(out[far]))
    near = np.abs(out.astype(D) - mean[0].astype(D)).max(1) < limit * CELL - slack
    assert np.array_equal(qt.bits(clamped[near]), qt.bits(out[near]))
    assert n[1] == 0
    # an unlimited move is taken too
    free, _ = qt.place(vertices, faces, mean[3], mean[0], grid[1], max_move=float("inf"))
    assert np.isfinite(free).all()
