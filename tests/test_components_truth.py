"""tests/components_truth.py held to properties nobody has to trust (no GPU, no library): the
labels are roots at or below their vertex, a face lies in one component, the number of components
is a breadth-first search's, the order of the faces and the names of the vertices do not matter,
and the counts add up."""
import numpy as np
import pytest

import components_truth as ct


def _meshes():
    out = [("nothing", np.zeros((0, 3), np.int32), 0), ("one vertex", np.zeros((0, 3), np.int32), 1),
           ("no faces", np.zeros((0, 3), np.int32), 5),
           ("one face", np.array([[0, 1, 2]], np.int32), 3)]
    for nv in (3, 64, 65, 257):
        out.append(("strip %d" % nv, ct.strip(nv), nv))
        out.append(("strip %d reversed" % nv, ct.reversed_ids(ct.strip(nv), nv), nv))
        out.append(("strip %d shuffled" % nv, ct.shuffled(ct.strip(nv), nv, nv)[0], nv))
    for hub_last in (False, True):
        f, nv = ct.star(200, hub_last)
        out.append(("star, hub last %s" % hub_last, f, nv))
    f, nv = ct.triangles(100)
    out.append(("triangles", ct.shuffled(f, nv, 1)[0], nv))
    f, nv = ct.tetrahedra(50)
    out.append(("tetrahedra", ct.shuffled(f, nv, 2)[0], nv))
    f, nv = ct.two_blobs(300, 3)
    out.append(("two blobs", f, nv))
    out.append(("two blobs, no bridge", f[:-1], nv))
    f, nv = ct.tetrahedra(60)
    out.append(("garbage", ct.with_garbage(f, nv, 4, 0.2)[0], nv))
    out.append(("degenerate", np.array([[4, 4, 4], [1, 1, 3], [5, 6, 6], [1, 1, 3]], np.int32), 9))
    return out


MESHES = _meshes()


@pytest.mark.parametrize("name,faces,nv", MESHES, ids=[m[0] for m in MESHES])
def test_the_truth_has_the_properties_of_the_definition(name, faces, nv):
    labels, vertex_counts, face_counts = ct.components(faces, nv)
    assert labels.shape == (nv,) and labels.dtype == np.int32
    assert vertex_counts.shape == (nv,) and face_counts.shape == (nv,)
    v = np.arange(nv)
    assert (labels <= v).all() and (labels >= 0).all()
    assert np.array_equal(labels[labels], labels)
    ok = ct.counted(faces, nv)
    inside = np.asarray(faces, np.int64).reshape(-1, 3)[ok]
    assert (labels[inside[:, 0]] == labels[inside[:, 1]]).all()
    assert (labels[inside[:, 1]] == labels[inside[:, 2]]).all()
    assert len(np.unique(labels)) == ct.bfs_count(faces, nv)
    # the counts
    assert int(face_counts.sum()) == int(ok.sum()) and int(vertex_counts.sum()) == nv
    is_root = labels == v
    assert (vertex_counts[~is_root] == 0).all() and (face_counts[~is_root] == 0).all()
    assert (vertex_counts[is_root] >= 1).all()
    # the smallest vertex of a component is its label
    for r in np.flatnonzero(is_root):
        assert np.flatnonzero(labels == r).min() == r
    # shuffling the faces changes nothing
    rng = np.random.default_rng(9)
    again = ct.components(np.asarray(faces).reshape(-1, 3)[rng.permutation(len(faces))], nv)
    for a, b in zip(again, (labels, vertex_counts, face_counts)):
        assert np.array_equal(a, b)
    # renumbering the vertices maps the partition onto itself
    order = rng.permutation(nv)
    renamed = ct.components(ct.renumber(faces, nv, order), nv)[0]
    if nv:
        same = labels[:, None] == labels[None, :] if nv <= 300 else None
        if same is not None:
            assert np.array_equal(renamed[order][:, None] == renamed[order][None, :], same)
        # the label of a class is the smallest new name in it
        for r in np.flatnonzero(is_root)[:50]:
            assert renamed[order[r]] == order[labels == r].min()


def test_the_expected_component_counts():
    assert len(np.unique(ct.labels_of(ct.strip(257), 257))) == 1
    f, nv = ct.two_blobs(300, 3)
    assert len(np.unique(ct.labels_of(f, nv))) == 1
    assert len(np.unique(ct.labels_of(f[:-1], nv))) == 2
    f, nv = ct.tetrahedra(50)
    labels, vc, fc = ct.components(f, nv)
    assert len(np.unique(labels)) == 50 and (vc[::4] == 4).all() and (fc[::4] == 4).all()
    # degenerate faces: (a, a, a) connects nothing and counts, (a, a, b) connects a and b
    labels, vc, fc = ct.components(np.array([[4, 4, 4], [1, 1, 3], [5, 6, 6], [1, 1, 3]]), 9)
    assert labels.tolist() == [0, 1, 2, 1, 4, 5, 5, 7, 8]
    assert fc.tolist() == [0, 2, 0, 0, 1, 1, 0, 0, 0] and vc.tolist() == [1, 2, 1, 0, 1, 2, 0, 1, 1]
    # a face with an index out of range is skipped whole
    labels, vc, fc = ct.components(np.array([[0, 1, 5], [2, -1, 3], [3, 4, 4]]), 5)
    assert labels.tolist() == [0, 1, 2, 3, 3] and fc.tolist() == [0, 0, 0, 1, 0]


def test_selection_and_compaction():
    n_faces = np.array([4, 0, 9, 4, 1, 9])
    assert ct.largest(n_faces, 3).tolist() == [2, 5, 0]
    assert ct.largest(n_faces, 10).tolist() == [2, 5, 0, 3, 4, 1]
    assert ct.select(n_faces, keep_largest=6).tolist() == [True, False, True, True, True, True]
    assert ct.select(n_faces, min_faces=4).tolist() == [True, False, True, True, False, True]
    assert ct.select(n_faces, min_fraction=0.5).tolist() == [False, False, True, False, False, True]
    assert ct.select(n_faces, min_fraction=4 / 9).tolist() == [True, False, True, True, False, True]
    assert ct.select(n_faces, min_faces=4, keep_largest=3).tolist() == \
        [True, False, True, False, False, True]
    assert ct.select(n_faces, min_faces=5, keep_largest=3).tolist() == \
        [False, False, True, False, False, True]
    vertices = np.arange(18, dtype=np.float32).reshape(6, 3)
    faces = np.array([[5, 3, 1], [0, 2, 4], [1, 3, 5]], np.int32)
    v, f, used = ct.compact(vertices, faces, [True, False, True])
    assert used.tolist() == [False, True, False, True, False, True]
    assert np.array_equal(v, vertices[[1, 3, 5]]) and f.tolist() == [[2, 1, 0], [0, 1, 2]]
    v, f, used, found, kept = ct.filtered(vertices, faces, keep_largest=1)
    assert (found, kept) == (2, 1) and f.tolist() == [[2, 1, 0], [0, 1, 2]]


def test_the_balls_are_four_closed_components():
    import isosurface_truth as it
    from fusion_truth import axes_of
    grid = (24, 22, 20)
    bbox = np.array([0, 0, 0, 2.4, 2.2, 2.0], np.float32)
    vertices, faces = it.extract(ct.balls_field(grid), 0.5, True, axes_of(bbox, grid), bbox)
    roots, component, n_vertices, n_faces = ct.dense(*ct.components(faces, len(vertices)))
    assert len(roots) == 4
    assert (n_faces == 2 * n_vertices - 4).all()            # each a closed surface of genus 0
    assert len(set(n_faces.tolist())) == 4 and n_faces.min() < 0.05 * n_faces.max()
