"""Connected components on the GPU: rn_mesh_components against
tests/components_truth.py -- labels, vertex_counts and face_counts EQUAL the truth's, integers
without a tolerance -- over the sizes at which a launch or the union-find can go wrong: strips
around the wavefront and the workgroup and one across many workgroups, stars that contend on one
word, many small pieces, degenerate and garbage faces; the entries behind the outputs, the status
word, three launches that give one array, the entry's refusals, the iso-surface of three balls
and a speck through SurfaceMesh.without_small_components, and the chain from ground-truth depth
maps of two spheres through the command line to a mesh without its floaters and the metrics."""
import ctypes
import os

import numpy as np
import pytest

import components_truth as ct
import mesh_harness as h

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
FILL = -7


def _launch(faces, nv, counts=True, status=True):
    """rn_mesh_components on device tensors, the outputs PAD entries longer than nv and prefilled
    -> (rc, labels, vertex_counts, face_counts, status) as host arrays, pads included, and faces
    on the device."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    f = h.cuda(np.reshape(faces, (-1, 3)), np.int32)
    outs = [h.padded(nv, FILL, torch.int32) for _ in range(3)]
    word = h.padded(1, FILL, torch.int32)
    rc = ctx.lib.rn_mesh_components(ctx._h, nv, len(f), _ptr(f), _ptr(outs[0]),
                                    _ptr(outs[1] if counts else None),
                                    _ptr(outs[2] if counts else None),
                                    _ptr(word if status else None), _stream())
    torch.cuda.synchronize()
    return (rc,) + tuple(o.cpu().numpy() for o in outs) + (word.cpu().numpy(), f)


def _same_as_truth(faces, nv, what, want=None):
    """The three arrays equal the truth's, the entries behind them keep their prefill, faces is
    what it was, status 0."""
    from raynet_amd import _lib
    want = ct.components(faces, nv) if want is None else want
    rc, labels, vc, fc, word, f_after = _launch(faces, nv)
    assert rc == _lib.RN_OK, what
    for got, name in ((labels, "labels"), (vc, "vertex_counts"), (fc, "face_counts")):
        h.assert_untouched(got, nv, FILL, (what, name))
    h.assert_untouched(word, 1, FILL, (what, "the status word"))
    h.assert_input_kept(f_after, np.reshape(faces, (-1, 3)), (what, "faces"))
    if nv == 0:
        assert word[0] == FILL, what                # no launch: nothing is written at all
    else:
        assert word[0] == 0, (what, "status", int(word[0]))
    for got, truth, name in zip((labels, vc, fc), want, ("labels", "vertex_counts", "face_counts")):
        assert got[:nv].dtype == np.int32
        assert np.array_equal(got[:nv], truth), \
            (what, name, int((got[:nv] != truth).sum()), np.flatnonzero(got[:nv] != truth)[:5])
    return labels[:nv], vc[:nv], fc[:nv]


# ------------------------------------------------------------------------------ a. sizes
NO_FACES = np.zeros((0, 3), np.int32)


@pytest.mark.parametrize("faces,nv", [(NO_FACES, 0), (NO_FACES, 1), (NO_FACES, 5),
                                      (np.array([[0, 1, 2]], np.int32), 3),
                                      (np.array([[4, 0, 2]], np.int32), 5)],
                         ids=["nv 0", "nv 1", "nv 5, no faces", "one face", "one face of five"])
def test_empty_and_trivial(faces, nv):
    labels, vc, fc = _same_as_truth(faces, nv, "trivial")
    if len(faces) == 0:
        assert np.array_equal(labels, np.arange(nv)) and (vc == 1).all() and (fc == 0).all()


@pytest.mark.parametrize("order", ["ascending", "reversed", "shuffled"])
@pytest.mark.parametrize("nv", [3, 64, 65, 256, 257, 20003])
def test_strips(nv, order):
    faces = ct.strip(nv)
    if order == "reversed":
        faces = ct.reversed_ids(faces, nv)
    elif order == "shuffled":
        faces, _ = ct.shuffled(faces, nv, seed=nv)
    labels, vc, fc = _same_as_truth(faces, nv, "strip %d %s" % (nv, order))
    assert (labels == 0).all() and vc[0] == nv and fc[0] == nv - 2


@pytest.mark.parametrize("hub_last", [False, True], ids=["vertex 0", "the last vertex"])
def test_contention_on_one_word(hub_last):
    faces, nv = ct.star(5000, hub_last)
    labels, vc, fc = _same_as_truth(faces, nv, "star")
    assert (labels == 0).all() and fc[0] == 5000 and vc[0] == nv


def test_many_small_pieces():
    faces, nv = ct.triangles(3000)
    faces, _ = ct.shuffled(faces, nv, seed=11)
    labels, vc, fc = _same_as_truth(faces, nv, "triangles")
    assert len(np.unique(labels)) == 3000 and set(vc.tolist()) == {0, 3} and set(fc.tolist()) == {0, 1}
    faces, nv = ct.tetrahedra(1000)
    faces, _ = ct.shuffled(faces, nv, seed=12)
    labels, vc, fc = _same_as_truth(faces, nv, "tetrahedra")
    assert len(np.unique(labels)) == 1000 and set(vc.tolist()) == {0, 4} and set(fc.tolist()) == {0, 4}


def test_two_blobs_joined_only_by_the_last_face():
    faces, nv = ct.two_blobs(4000, seed=13)
    apart = _same_as_truth(faces[:-1], nv, "two blobs apart")[0]
    assert len(np.unique(apart)) == 2
    labels, vc, fc = _same_as_truth(faces, nv, "two blobs and the bridge")
    assert (labels == 0).all() and fc[0] == 8001


def test_degenerate_and_duplicate_faces_and_loose_vertices():
    faces = np.array([[4, 4, 4], [1, 1, 3], [5, 6, 6], [1, 1, 3], [8, 8, 8]], np.int32)
    labels, vc, fc = _same_as_truth(faces, 10, "degenerate")
    assert labels.tolist() == [0, 1, 2, 1, 4, 5, 5, 7, 8, 9]
    assert fc.tolist() == [0, 2, 0, 0, 1, 1, 0, 0, 1, 0]
    # every face twice: the labels stay, the face counts double
    base, nv = ct.tetrahedra(300)
    base, _ = ct.shuffled(base, nv, seed=14)
    once = ct.components(base, nv)
    twice = _same_as_truth(np.concatenate([base, base]), nv, "duplicates")
    assert np.array_equal(twice[0], once[0]) and np.array_equal(twice[2], 2 * once[2])
    # vertices in no face, in between: pieces on every third block of ids
    parts = [np.asarray(ct.strip(50), np.int64) + 150 * k for k in range(20)]
    labels, vc, fc = _same_as_truth(np.concatenate(parts), 3000, "loose vertices")
    assert len(np.unique(labels)) == 20 + 3000 - 20 * 50 and (fc[vc == 1] == 0).all()


def test_garbage_faces_are_skipped_whole():
    for name, (faces, nv) in (("tetrahedra", ct.tetrahedra(700)), ("strip", (ct.strip(3001), 3001)),
                              ("star", ct.star(2000))):
        faces, _ = ct.shuffled(faces, nv, seed=15)
        planted, hit = ct.with_garbage(faces, nv, seed=16)
        assert 0.02 * len(faces) < hit.sum() < 0.1 * len(faces)
        assert not ct.counted(planted, nv)[hit].any() and ct.counted(planted, nv)[~hit].all()
        got = _same_as_truth(planted, nv, "garbage in " + name)
        # ... and change no other entry: the result is that of the mesh without them
        for a, b in zip(got, ct.components(faces[~hit], nv)):
            assert np.array_equal(a, b), name
    # nothing but garbage
    bad = np.array([[-1, 0, 1], [0, 5, 1], [2 ** 31 - 1, 0, 1], [0, 1, -2 ** 31]], np.int64)
    labels, vc, fc = _same_as_truth(bad.astype(np.int32), 5, "only garbage")
    assert np.array_equal(labels, np.arange(5)) and (fc == 0).all()


def test_three_launches_give_one_array():
    from raynet_amd import _lib
    strip, _ = ct.shuffled(ct.strip(20003), 20003, seed=20003)
    star, nv_star = ct.star(5000)
    for faces, nv in ((strip, 20003), (star, nv_star)):
        runs = [_launch(faces, nv) for _ in range(3)]
        for run in runs:
            assert run[0] == _lib.RN_OK and run[4][0] == 0
        for run in runs[1:]:
            for a, b in zip(run[1:4], runs[0][1:4]):
                assert np.array_equal(a, b)


def test_counts_and_status_are_optional():
    from raynet_amd import _lib
    faces, nv = ct.tetrahedra(100)
    want = ct.components(faces, nv)
    rc, labels, vc, fc, word = _launch(faces, nv, counts=False, status=False)[:5]
    assert rc == _lib.RN_OK and np.array_equal(labels[:nv], want[0])
    assert (vc == FILL).all() and (fc == FILL).all() and (word == FILL).all()
    rc, labels, vc, fc, word = _launch(faces, nv, counts=True, status=False)[:5]
    assert rc == _lib.RN_OK and np.array_equal(vc[:nv], want[1]) and np.array_equal(fc[:nv], want[2])
    assert (word == FILL).all()


# ------------------------------------------------------------------------------ b. a real mesh
def test_the_iso_surface_of_three_balls_and_a_speck():
    import torch
    from raynet_amd.fusion import _grid_context
    from raynet_amd.volume import SurfaceMesh
    grid = (24, 22, 20)
    bbox = np.array([0, 0, 0, 2.4, 2.2, 2.0], F)
    ctx = _grid_context(bbox, grid)
    vertices, faces = ctx.isosurface(torch.from_numpy(ct.balls_field(grid)).cuda(), 0.5, True)
    vertices, faces = vertices.cpu().numpy(), faces.cpu().numpy()
    truth = ct.components(faces, len(vertices))
    roots, component, n_vertices, n_faces = ct.dense(*truth)
    assert len(roots) == 4 and (n_faces == 2 * n_vertices - 4).all()      # four closed surfaces
    _same_as_truth(faces, len(vertices), "balls", truth)
    rng = np.random.default_rng(5)
    normals = rng.normal(size=vertices.shape).astype(F)
    colors = rng.integers(0, 256, size=vertices.shape).astype(np.uint8)
    mesh = SurfaceMesh(vertices, faces, normals, colors)
    found = mesh.components()
    assert np.array_equal(found.labels, truth[0]) and np.array_equal(found.roots, roots)
    assert np.array_equal(found.n_faces, n_faces) and np.array_equal(found.n_vertices, n_vertices)
    assert np.array_equal(found.component, component)
    speck = int(n_faces.min())
    print("balls: %d vertices, %d faces, components of %s faces" % (
        len(vertices), len(faces), n_faces.tolist()))
    for kw, kept in ((dict(keep_largest=1), 1), (dict(keep_largest=2), 2),
                     (dict(min_faces=speck + 1), 3), (dict(min_fraction=0.5), None)):
        got = mesh.without_small_components(**kw)
        want_v, want_f, used, K, k = ct.filtered(vertices, faces, **kw)
        assert K == 4 and (kept is None or k == kept) and 0 < len(want_f) < len(faces), kw
        assert np.array_equal(got.vertices.view(np.int32), want_v.view(np.int32)), kw
        assert np.array_equal(got.faces, want_f), kw
        assert np.array_equal(got.normals, normals[used]) and np.array_equal(got.colors, colors[used])
    largest = int(np.argmax(n_faces))
    one = mesh.keep_components([largest])
    assert np.array_equal(one.faces, mesh.without_small_components(keep_largest=1).faces)
    assert len(one.faces) == n_faces[largest] and len(one.vertices) == n_vertices[largest]


# ------------------------------------------------------------------------------ c. refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    faces_np, nv = ct.tetrahedra(10)
    faces = torch.from_numpy(faces_np).cuda()
    outs = [torch.full((nv,), FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    word = torch.full((1,), FILL, dtype=torch.int32, device="cuda")
    #       0   1            2             3              4              5              6
    good = [nv, len(faces), _ptr(faces), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(word)]
    for at_, value in [(0, -1), (1, -1), (0, 2 ** 31 - 1), (0, 2 ** 40), (1, (2 ** 31 - 1) // 3 + 1),
                       (1, 2 ** 40), (3, null), (2, null)]:
        args = list(good)
        args[at_] = value
        assert ctx.lib.rn_mesh_components(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_mesh_components" in last(ctx._h)
    torch.cuda.synchronize()
    assert all((o == FILL).all() for o in outs) and (word == FILL).all()
    # what is NOT refused: no faces and no pointer to them; nothing at all
    assert ctx.lib.rn_mesh_components(ctx._h, nv, 0, null, *good[3:], _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), np.arange(nv)) and int(word.item()) == 0
    assert (outs[1] == 1).all() and (outs[2] == 0).all()
    assert ctx.lib.rn_mesh_components(ctx._h, 0, 0, null, null, null, null, null, _stream()) == _lib.RN_OK
    # the wrapper: what it returns, and tensors that are not what the kernels read
    labels, vc, fc = ctx.mesh_components(faces, nv)
    want = ct.components(faces_np, nv)
    for got, truth in zip((labels, vc, fc), want):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), truth)
    given = ctx.mesh_components(faces, nv, labels=outs[0], vertex_counts=outs[1], face_counts=outs[2])
    assert given[0] is outs[0] and np.array_equal(outs[2].cpu().numpy(), want[2])
    for bad, match in [
            (dict(faces=faces.long()), "faces"), (dict(faces=faces[:, :2]), "faces"),
            (dict(faces=faces.t().contiguous().t()), "faces"), (dict(faces=faces.cpu()), "faces"),
            (dict(faces=faces.reshape(-1)), "faces"), (dict(n_vertices=-1), "n_vertices"),
            (dict(labels=outs[0][:-1]), "labels"), (dict(labels=outs[0].long()), "labels"),
            (dict(vertex_counts=outs[1][::2]), "vertex_counts"),
            (dict(face_counts=outs[2].float()), "face_counts")]:
        kw = dict(faces=faces, n_vertices=nv)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ctx.mesh_components(**kw)


# ------------------------------------------------------------------------------ d. the chain
def test_from_ground_truth_maps_of_two_spheres_to_a_mesh_without_floaters(tmp_path, capsys):
    from raynet_amd.common.mesh_io import parse_stl_file_to_pointcloud
    from raynet_amd.common.scene import get_scene
    from raynet_amd.fusion import fuse_scene
    from raynet_amd.pointcloud import Pointcloud
    from raynet_amd.scripts import compute_metrics, fuse_depth_maps
    from raynet_amd.volume import SurfaceMesh
    # (the spheres' surfaces are 0.36 apart, the truncation below is 0.25)
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps()
    scene_dir, preds = str(tmp_path / "scene"), str(tmp_path / "predictions")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    os.makedirs(preds)
    on_disk = get_scene("restrepo", scene_dir)
    common = ["--gt", "--truncation", "0.25", "--start_end", "0,3", "--grid_shape", "18,22,14"]
    # without the new flags: the bytes of the API without a filter, and no tally
    plain, api = str(tmp_path / "plain.ply"), str(tmp_path / "api.ply")
    assert fuse_depth_maps.main([scene_dir, preds, plain] + common) == 0
    assert "components:" not in capsys.readouterr().out
    volume = fuse_scene(on_disk, [on_disk.get_depth_map(i) for i in range(3)], [0, 1, 2], grid,
                        trunc=0.25)
    whole = volume.mesh()
    whole.save_ply(api)
    assert open(plain, "rb").read() == open(api, "rb").read()
    # the truth on that mesh: the large sphere's component and the floaters
    want_v, want_f, used, K, k = ct.filtered(whole.vertices, whole.faces, keep_largest=1)
    roots, component, n_vertices, n_faces = ct.dense(*ct.components(whole.faces, len(whole.vertices)))
    assert K >= 2 and k == 1 and 0 < len(want_f) < len(whole.faces)
    print("fused: %d faces in %d components of %s faces" % (len(whole.faces), K, n_faces.tolist()))
    # --keep_largest 1
    kept_ply, cloud_ply = str(tmp_path / "kept.ply"), str(tmp_path / "kept_cloud.ply")
    assert fuse_depth_maps.main([scene_dir, preds, kept_ply, "--keep_largest", "1", "--normals",
                                 "--mesh_cloud", cloud_ply, "--mesh_samples", "2000",
                                 "--seed", "3"] + common) == 0
    assert "components: %d found, 1 kept, %d -> %d faces\n" % (K, len(whole.faces), len(want_f)) \
        in capsys.readouterr().out
    kept = SurfaceMesh.load_ply(kept_ply)
    assert np.array_equal(kept.faces, want_f)
    assert np.array_equal(kept.vertices.view(np.int32), want_v.view(np.int32))
    assert kept.normals is not None and kept.normals.shape == want_v.shape
    # ... which is the large sphere's: every vertex within the truncation (times the factor of the
    # sqrt-free distance, z > 2 here) and a cell diagonal of it, none near the small one
    cell = (bbox[3:] - bbox[:3]).astype(D) / np.array(grid)
    r = np.sqrt(((kept.vertices.astype(D) - np.array(big[0])) ** 2).sum(1))
    assert np.abs(r - big[1]).max() <= 0.25 * (1 + 0.25 / 4) + float(np.sqrt((cell ** 2).sum()))
    # "near the small one": within twice its radius of its centre.  The small sphere's own shell
    # is among what was dropped, and no kept vertex is near it (the restatement on the CPU has the
    # nearest kept vertex 0.50 from that centre, and 60 of the 73 dropped vertices within 0.30)
    near = 2 * small[1]
    gone = whole.vertices[~used].astype(D)
    assert len(gone) == len(whole.vertices) - len(kept.vertices)
    assert len(kept.vertices) == int(n_vertices.max())
    to_small = np.sqrt(((gone - np.array(small[0])) ** 2).sum(1))
    assert (to_small < near).sum() >= 10
    assert np.sqrt(((kept.vertices.astype(D) - np.array(small[0])) ** 2).sum(1)).min() > near
    # the cloud is sampled from the filtered mesh and goes into the accuracy metric.  (The one
    # comparison of this file that is no equality: the samples are float32 points of a file, at
    # barycentric positions on triangles, so their float64 distance to the mesh is rounding and
    # not 0; 1e-5 of the box's largest coordinate, 1 here, is the bound tests/test_fusion_gpu.py
    # uses for the same statement.  A sample of a dropped floater would be 0.1 and more away.)
    cli_points = parse_stl_file_to_pointcloud(cloud_ply)
    assert cli_points.shape == (2000, 3)
    dist, _, _ = kept.raycaster().closest_points(cli_points)
    assert float(dist.max()) <= 1e-5
    args = compute_metrics.build_parser().parse_args(
        [scene_dir, str(tmp_path), "accuracy", "--use_pc_from_depthmap", "--borders", "4"])
    values, _ = compute_metrics.build_metric("accuracy", args).compute(
        on_disk, [0, 1], None, Pointcloud(np.ascontiguousarray(cli_points.T)))
    assert np.asarray(values).size == 2000 and np.isfinite(values).all()
    # the other two flags reach the same filter
    for flags, kw in ((["--min_component_faces", "10"], dict(min_faces=10)),
                      (["--min_component_fraction", "0.5"], dict(min_fraction=0.5))):
        path = str(tmp_path / "other.ply")
        assert fuse_depth_maps.main([scene_dir, preds, path] + flags + common) == 0
        v, f, _, _, k = ct.filtered(whole.vertices, whole.faces, **kw)
        assert "%d kept, %d -> %d faces" % (k, len(whole.faces), len(f)) in capsys.readouterr().out
        again = SurfaceMesh.load_ply(path)
        assert np.array_equal(again.faces, f) and np.array_equal(again.vertices.view(np.int32),
                                                                 v.view(np.int32))
