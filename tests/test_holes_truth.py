"""The two restatements of rn_mesh_fill_holes in tests/holes_truth.py (no GPU): the Python loop and
the vectorised one agree to the bit on every mesh the kernels are tested on, and the filled meshes
have the properties the definition promises."""
import numpy as np
import pytest

import holes_truth as ht
import smooth_truth as st

F = np.float32
CASES = ht.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_the_loop_and_the_vectorised_truth_agree_to_the_bit(name):
    vertices, faces, max_edges = CASES[name]
    plain, fast = ht.fill_plain(vertices, faces, max_edges), ht.fill(vertices, faces, max_edges)
    assert ht.same(plain, fast), name
    assert fast[0].dtype == F and fast[1].dtype == np.int32 and fast[2].dtype == np.int32
    assert fast[3].dtype == np.int64 and fast[3].shape == (5,)
    k, m, loops, not_simple, half = fast[3].tolist()
    assert (k, m) == (len(fast[0]), len(fast[1])) and k == len(fast[2])
    assert k + not_simple <= loops and m <= half and (np.diff(fast[2]) > 0).all()
    # the same with the faces in another order: the loops are the same sets, so are the counts,
    # the sources and the centres' sums up to the walk's start -- which is the label either way
    shuffled = ht.fill(vertices, ht.permuted(faces), max_edges)
    assert np.array_equal(shuffled[3], fast[3]) and np.array_equal(shuffled[2], fast[2])
    assert np.array_equal(shuffled[0].view(np.uint32), fast[0].view(np.uint32))
    assert np.array_equal(shuffled[1], fast[1])


def test_the_smallest_loop_is_a_triangle():
    vertices, faces = ht.open_tetrahedron()
    new_vertices, new_faces, source, counts = ht.fill(vertices, faces, 3)
    assert counts.tolist() == [1, 3, 1, 0, 3] and source.tolist() == [1]
    assert np.array_equal(new_faces, [[2, 1, 4], [3, 2, 4], [1, 3, 4]])
    out_v, out_f, _, stats = ht.filled_mesh(vertices, faces, 3)
    assert ht.is_closed(out_f) and not st.boundary_vertices(out_f, len(out_v)).any()
    assert stats == dict(filled=1, new_faces=3, loops=1, not_simple=0, boundary_edges=3)


@pytest.mark.parametrize("n", [3, 63, 64, 65, 300])
def test_a_tube_gets_both_ends_capped(n):
    vertices, faces = ht.tube(n)
    new_vertices, new_faces, source, counts = ht.fill(vertices, faces, n)
    assert counts.tolist() == [2, 2 * n, 2, 0, 2 * n] and source.tolist() == [0, n]
    out_v, out_f, _, _ = ht.filled_mesh(vertices, faces, n)
    assert ht.is_closed(out_f) and not st.boundary_vertices(out_f, len(out_v)).any()
    # the centre is the mean of the ring, to the rounding of one fp64 sum
    for k, ring in enumerate((vertices[:n], vertices[n:])):
        mean = ring.astype(np.float64).mean(0)
        assert np.abs(new_vertices[k].astype(np.float64) - mean).max() <= 1e-6
    # the walk follows the boundary half-edges (ring 0 upwards, ring 1 downwards) and every new
    # face runs against its half-edge
    assert new_faces[0].tolist() == [1, 0, 2 * n] and new_faces[n].tolist() == [2 * n - 1, n, 2 * n + 1]
    if n > 3:
        assert ht.fill(vertices, faces, n - 1)[3].tolist() == [0, 0, 2, 0, 2 * n]


def test_the_punched_sheet_keeps_its_rim():
    vertices, faces = ht.punched_sheet()
    assert len(vertices) == 13 * 10 and len(faces) == 2 * (12 * 9 - 5)
    new_vertices, new_faces, source, counts = ht.fill(vertices, faces, 10)
    assert counts.tolist() == [3, 16, 4, 0, 16 + 42] and source.tolist() == [28, 48, 71]
    out_v, out_f, _, _ = ht.filled_mesh(vertices, faces, 10)
    rim = st.boundary_vertices(out_f, len(out_v))
    x, y = np.arange(len(vertices)) % 13, np.arange(len(vertices)) // 13
    assert np.array_equal(rim[:len(vertices)], (x == 0) | (x == 12) | (y == 0) | (y == 9))
    assert not rim[len(vertices):].any()
    # every new face is wound like the sheet: its normal points to +z
    tri = out_v[new_faces].astype(np.float64)
    assert (np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])[:, 2] > 0).all()
    # max_edges = 3 fills only triangles: there are none
    assert ht.fill(vertices, faces, 3)[3].tolist() == [0, 0, 4, 0, 58]
    # a second application adds nothing
    again = ht.fill(out_v, out_f, 10)
    assert again[3].tolist() == [0, 0, 1, 0, 42] and len(again[0]) == 0 and len(again[1]) == 0
    # with max_edges at least the rim's length the rim is capped too
    everything = ht.filled_mesh(vertices, faces, 42)
    assert everything[3]["filled"] == 4 and everything[3]["new_faces"] == 58
    assert everything[2].tolist() == [0, 28, 48, 71] and ht.is_closed(everything[1])
    assert ht.fill(vertices, faces, 41)[3].tolist() == [3, 16, 4, 0, 58]


def test_two_holes_that_meet_at_a_vertex_stay_open():
    vertices, faces = ht.bow_tie_sheet()
    new_vertices, new_faces, source, counts = ht.fill(vertices, faces, 10)
    assert counts.tolist() == [1, 4, 3, 1, 4 + 8 + 32] and source.tolist() == [1 * 9 + 6]
    # not even when every length is allowed: the bow-tie is one loop of 8 edges that is not simple
    assert ht.fill(vertices, faces, 65536)[3].tolist() == [2, 36, 3, 1, 44]


@pytest.mark.parametrize("name,open_edges", [("flipped_rim", 4), ("nan_rim", 4), ("doubled_face", 3)])
def test_loops_that_stay_open(name, open_edges):
    vertices, faces, max_edges = CASES[name]
    new_vertices, new_faces, source, counts = ht.fill(vertices, faces, max_edges)
    assert counts.tolist() == [2, 12, 4, 1, 12 + 42 + open_edges] and source.tolist() == [28, 48]
    assert ht.fill(vertices, faces, 65536)[3][0] == 3         # the rim, not the loop of cell (6, 5)


def test_faces_that_do_not_count_are_ignored():
    vertices, faces = ht.punched_sheet()
    dirty = ht.with_garbage(faces, len(vertices))
    assert len(dirty) == len(faces) + 8 and not ht.counting(dirty, len(vertices)).all()
    clean, got = ht.fill(vertices, faces, 10), ht.fill(vertices, dirty, 10)
    assert np.array_equal(got[3], clean[3]) and np.array_equal(got[2], clean[2])
    assert np.array_equal(got[0].view(np.uint32), clean[0].view(np.uint32))
    assert np.array_equal(got[1], clean[1])
    offsets, corners = ht.corner_table(dirty, len(vertices))
    flat = dirty.reshape(-1).astype(np.int64)
    for v in (0, 5, 71, len(vertices) - 1):
        row = corners[offsets[v]:offsets[v + 1]]
        assert (flat[row] == v).all() and (np.diff(row) > 0).all()
    assert offsets[-1] == ((flat >= 0) & (flat < len(vertices))).sum()


def test_the_cut_ball_is_open_where_the_grid_ends():
    vertices, faces, max_edges = CASES["cut_ball"]
    new_vertices, new_faces, source, counts = ht.fill(vertices, faces, max_edges)
    rim = st.boundary_vertices(faces, len(vertices))
    assert rim.any() and counts[2] >= 1 and counts[4] == rim.sum()
    out_v, out_f, _, stats = ht.filled_mesh(vertices, faces, 65536)
    assert stats["filled"] + stats["not_simple"] == stats["loops"]
    if stats["not_simple"] == 0:
        assert ht.is_closed(out_f)
