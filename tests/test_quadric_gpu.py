"""Quadric-error placement on the GPU: rn_mesh_place_quadric against
tests/quadric_truth.py -- positions_out and counts EQUAL the truth's bits, the four inputs are what
they were, the rows behind nvo and the bytes behind the workspace keep their prefill -- over the
sizes at which a launch can go wrong: no output vertex, no faces, one triangle in three cells, a
tetrahedron, strips around the wavefront and the workgroup, five thousand faces into one cluster
and into five thousand, the rotated cube (and the quality relation on the GPU's own output),
anisotropic cells, garbage in the faces, the positions and the clustering, three launches that give
one result, the entry's refusals, the wrapper, and the chain from the depth maps of two spheres
through the command line."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mesh_harness as h
import quadric_truth as qt
import simplify_truth as sp
from conftest import REPO
from test_quadric_cpu import garbage_case

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
I = np.int32
FILL = -7.5
NO_FACES = np.zeros((0, 3), I)


def _cell3(cell):
    return (ctypes.c_double * 3)(*[float(x) for x in np.broadcast_to(np.asarray(cell, D), (3,))])


def _launch(vertices, faces, cluster, positions, cell, regularization, max_move):
    """rn_mesh_place_quadric on device tensors, positions_out PAD rows longer than nvo and the
    workspace TAIL bytes longer than reported, both prefilled -> (rc, positions_out, counts, the
    four inputs on the device, the workspace, the bytes it needs)."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    nv, nf, nvo = len(vertices), len(faces), len(positions)
    v, f = h.cuda(np.reshape(vertices, (-1, 3)), F), h.cuda(np.reshape(faces, (-1, 3)), I)
    c, p = h.cuda(cluster, I), h.cuda(np.reshape(positions, (-1, 3)), F)
    need = int(ctx.lib.rn_mesh_place_quadric_workspace_bytes(nv, nf, nvo))
    assert need == 88 * nvo
    work = h.workspace(need)
    out = h.padded((nvo, 3), FILL, torch.float32)
    counts = h.padded(2, -77, torch.int64)
    rc = ctx.lib.rn_mesh_place_quadric(ctx._h, nv, _ptr(v), nf, _ptr(f), _ptr(c), nvo, _ptr(p),
                                       _cell3(cell), float(regularization), float(max_move),
                                       _ptr(out), _ptr(counts), _ptr(work), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), counts.cpu().numpy(), (v, f, c, p), work, need


def _same_as_truth(vertices, faces, cluster, positions, cell, what, regularization=qt.REGULARIZATION,
                   max_move=qt.MAX_MOVE, want=None):
    """positions_out and counts have the truth's bits, the inputs their own, the pads their
    prefill -> (the truth's positions, its counts)."""
    from raynet_amd import _lib
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, I).reshape(-1, 3)
    cluster = np.ascontiguousarray(cluster, I).reshape(-1)
    positions = np.ascontiguousarray(positions, F).reshape(-1, 3)
    nvo = len(positions)
    if want is None:
        want = qt.place(vertices, faces, cluster, positions, cell, regularization, max_move)
    rc, out, counts, inputs, work, need = _launch(vertices, faces, cluster, positions, cell,
                                                  regularization, max_move)
    assert rc == _lib.RN_OK, what
    h.assert_untouched(counts, 2, -77, (what, "counts"))
    h.assert_untouched(out, nvo, FILL, (what, "positions_out"))
    h.assert_untouched(work, need, h.TAIL_BYTE, (what, "the workspace"))
    for tensor, before, name in zip(inputs, (vertices, faces, cluster, positions),
                                    ("vertices_in", "faces_in", "cluster", "positions_in")):
        h.assert_input_kept(tensor, before, (what, name))
    h.assert_same_bits(out[:nvo], want[0], what)
    assert counts[:2].tolist() == want[1].tolist(), (what, counts[:2], want[1])
    return want


def _clustered(vertices, faces, cell):
    """The clustering the placement follows, by its truth -> (cluster, mean positions, cell [3])."""
    grid = sp.grid_around(vertices, cell)
    mean = sp.simplify(vertices, faces, *grid)
    return mean[3], mean[0], grid[1]


@pytest.fixture(scope="module")
def cube():
    vertices, faces = qt.rotated_cube(6)
    cluster, positions, cell = _clustered(vertices, faces, 0.4)
    assert len(positions) == 48
    return vertices, faces, cluster, positions, cell


# ------------------------------------------------------------------------------ a. sizes
def test_no_output_vertex_writes_only_the_counts():
    tetra = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], I)
    want = _same_as_truth(tetra, faces, np.full(4, -1, I), np.zeros((0, 3), F), 1.0, "nvo 0")
    assert want[1].tolist() == [0, 0]


def test_no_faces_keep_every_bit():
    vertices = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [1.5, 0.5, 0.5], [1.25, 0.25, 0.75]], F)
    positions = np.array([[0.25, 0.35, 0.45], [1.375, 0.375, 0.625]], F)
    want = _same_as_truth(vertices, NO_FACES, np.array([0, 0, 1, 1], I), positions, 1.0, "no faces")
    assert np.array_equal(h.bits(want[0]), h.bits(positions)) and want[1].tolist() == [0, 2]


def test_one_triangle_in_three_cells_keeps_its_bits():
    tri = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.5], [0.25, 0.75, 0.5]], F)
    face = np.array([[0, 1, 2]], I)
    cluster, positions, cell = _clustered(tri, face, 0.5)
    assert cluster.tolist() == [0, 1, 2]
    want = _same_as_truth(tri, face, cluster, positions, cell, "singletons")
    assert np.array_equal(h.bits(want[0]), h.bits(tri)) and want[1].tolist() == [0, 0]


def test_one_tetrahedron():
    tetra = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], I)
    moved = _same_as_truth(tetra, faces, np.array([0, 0, 1, 2], I),
                           np.array([[0.5, 0, 0], [0, 1, 0], [0, 0, 1]], F), (1.0, 0.5, 2.0),
                           "two in a cluster")
    assert moved[1].tolist() == [1, 0]
    _same_as_truth(tetra, faces, np.zeros(4, I), np.array([[0.25, 0.25, 0.25]], F), 1.0,
                   "one cluster", regularization=2.0 ** -20, max_move=float("inf"))


@pytest.mark.parametrize("nf", [63, 64, 65, 255, 256, 257])
def test_strips(nf):
    """One wavefront and one workgroup of faces, one less and one more; cells of 1 and of 3.5
    spacings of the ridge, which runs through every cluster."""
    vertices, faces = qt.ridge_strip(nf + 2, seed=nf)
    assert len(faces) == nf
    for cell in (1.0, 3.5):
        cluster, positions, cell3 = _clustered(vertices, faces, cell)
        want = _same_as_truth(vertices, faces, cluster, positions, cell3, (nf, cell))
        assert want[1][0] > 0


def test_five_thousand_faces_into_one_cluster_and_into_five_thousand():
    """Contention on ten words; then none at all."""
    vertices, faces = qt.fan(5000, seed=2)
    cluster = np.zeros(len(vertices), I)
    positions = vertices.astype(D).mean(0, keepdims=True).astype(F)
    want = _same_as_truth(vertices, faces, cluster, positions, 1.0, "one cluster")
    assert want[1].tolist() == [1, 0]
    S = qt.sums(vertices, faces, cluster, positions, 1.0)
    assert S[0, 10] == len(vertices) == 5002 and (S[0, :10] != 0).all()
    vertices, faces, cluster, positions = qt.spread_faces(5000, seed=3)
    want = _same_as_truth(vertices, faces, cluster, positions, 1.0, "5000 clusters")
    assert want[1].tolist() == [5000, 0]


# ------------------------------------------------------------------------------ b. surfaces
def test_the_rotated_cube_and_the_quality_relation_on_the_gpus_output(cube):
    vertices, faces, cluster, positions, cell = cube
    _same_as_truth(vertices, faces, cluster, positions, cell, "cube")
    rc, out, counts, _, _, _ = _launch(vertices, faces, cluster, positions, cell, 2.0 ** -10, 1.0)
    at_mean, at_quadric = qt.cube_distance(positions) / 0.4, qt.cube_distance(out[:48]) / 0.4
    rms = [float(np.sqrt((d ** 2).mean())) for d in (at_mean, at_quadric)]
    print("rotated cube on the GPU, in cell sides: mean RMS %.3e (max %.3e), quadric RMS %.3e "
          "(max %.3e)" % (rms[0], at_mean.max(), rms[1], at_quadric.max()))
    assert rms[1] < rms[0] and (at_quadric <= at_mean + 1e-6).all()
    _same_as_truth(vertices, faces, cluster, positions, cell, "held", regularization=1.0)
    _same_as_truth(vertices, faces, cluster, positions, cell, "clamped", max_move=0.05)


def test_anisotropic_cells(cube):
    vertices, faces = cube[:2]
    for cell in ((0.4, 0.2, 0.3), (0.15, 0.6, 0.3)):
        cluster, positions, cell3 = _clustered(vertices, faces, cell)
        want = _same_as_truth(vertices, faces, cluster, positions, cell3, cell, max_move=0.25)
        assert want[1][0] > 0
        moved = np.abs(want[0].astype(D) - positions.astype(D)) / cell3
        assert moved.max() <= 0.25 + 1e-6 and moved.max() > 0.2         # the clamp is per axis


# ------------------------------------------------------------------------------ c. garbage
def test_garbage_reads_and_writes_nothing_out_of_bounds():
    """Face indices out of range, NaN and infinite vertices, a face without area, cluster entries
    of -1 and beyond nvo, a position far from its members, a huge triangle and a tiny one."""
    vertices, faces, cluster, positions, cell = garbage_case()
    want = _same_as_truth(vertices, faces, cluster, positions, cell, "garbage")
    assert want[1][0] > 0 and want[1][1] > 0
    # every cluster entry and every face index garbage: nothing moves
    bad = np.full(len(vertices), 2 ** 31 - 1, I)
    bad[::2] = -2 ** 31
    still = _same_as_truth(vertices, faces, bad, positions, cell, "no cluster")
    assert np.array_equal(h.bits(still[0]), h.bits(positions)) and still[1].tolist() == [0, 0]
    _same_as_truth(vertices, np.full_like(faces, -1), cluster, positions, cell, "no face")
    nothing = np.full_like(vertices, np.nan)
    _same_as_truth(nothing, faces, cluster, positions, cell, "all NaN")
    _same_as_truth(vertices, faces, cluster, np.full_like(positions, np.inf), cell, "positions inf")


def test_three_launches_give_one_result(cube):
    want = qt.place(*cube)
    for run in range(3):
        _same_as_truth(*cube, what=run, want=want)


# ------------------------------------------------------------------------------ d. refusals
def test_bad_arguments_are_refused_before_any_launch(cube):
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    from raynet_amd.simplify import simplify_mesh
    ctx = h.ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    vertices, faces, cluster, positions, cell = cube
    nv, nf, nvo = len(vertices), len(faces), len(positions)
    v, f, c, p = h.cuda(vertices, F), h.cuda(faces, I), h.cuda(cluster, I), h.cuda(positions, F)
    need = int(ctx.lib.rn_mesh_place_quadric_workspace_bytes(nv, nf, nvo))
    work = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((nvo, 3), FILL, dtype=torch.float32, device="cuda")
    counts = torch.full((2,), -77, dtype=torch.int64, device="cuda")

    def at_(pointer, byte):
        return ctypes.c_void_p(pointer.value + byte)

    def three(k, bad):
        values = [float(x) for x in cell]
        values[k] = bad
        return _cell3(values)

    #       0   1        2   3        4        5    6        7            8           9
    good = [nv, _ptr(v), nf, _ptr(f), _ptr(c), nvo, _ptr(p), _cell3(cell), 2.0 ** -10, 1.0,
            _ptr(out), _ptr(counts), _ptr(work)]    # 10, 11, 12
    nan, inf = float("nan"), float("inf")
    cases = [(0, -1), (2, -1), (0, 2 ** 31 - 1), (0, 2 ** 40), (2, (2 ** 31 - 1) // 3 + 1),
             (2, 2 ** 40), (5, -1), (5, nv + 1), (5, 2 ** 40), (1, null), (3, null), (4, null),
             (6, null), (7, null), (10, null), (11, null), (12, null),
             (12, at_(_ptr(work), 4)), (12, at_(_ptr(work), 1)),
             (10, _ptr(v)), (10, _ptr(f)), (10, _ptr(c)), (10, _ptr(p)), (10, _ptr(work)),
             (8, 0.0), (8, -1.0), (8, 2.0 ** -21), (8, 1.0 + 2.0 ** -52), (8, nan), (8, inf),
             (9, 0.0), (9, -1.0), (9, nan), (9, -inf)]
    for k in range(3):
        cases += [(7, three(k, x)) for x in (0.0, -1.0, nan, inf)]
    for where, value in cases:
        args = list(good)
        args[where] = value
        assert ctx.lib.rn_mesh_place_quadric(ctx._h, *args, _stream()) == INVALID, (where, value)
        assert b"rn_mesh_place_quadric" in last(ctx._h), (where, value)
    assert ctx.lib.rn_mesh_place_quadric(None, *good, _stream()) == INVALID
    fn = ctx.lib.rn_mesh_place_quadric_workspace_bytes
    assert fn(-1, 0, 0) == -1 and fn(0, 2 ** 40, 0) == -1 and fn(2 ** 31 - 1, 0, 0) == -1
    assert fn(4, 2, 5) == -1 and fn(4, 2, -1) == -1
    torch.cuda.synchronize()
    assert (out == FILL).all() and (work == 0xA5).all() and (counts == -77).all()
    assert np.array_equal(h.bits(v.cpu().numpy()), h.bits(vertices))
    # what is NOT refused: no output vertex and no pointers but counts; no faces and no pointer to
    # them; max_move inf; the regulariser at both ends; a workspace moved by eight bytes
    assert ctx.lib.rn_mesh_place_quadric(ctx._h, nv, null, nf, null, null, 0, null, _cell3(cell),
                                         2.0 ** -10, 1.0, null, _ptr(counts), null,
                                         _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0] and (out == FILL).all()
    want = qt.place(vertices, faces, cluster, positions, cell)
    for where, value in [(9, inf), (8, 2.0 ** -20), (8, 1.0), (12, at_(_ptr(work), 8)), (3, null)]:
        args = list(good)
        args[where] = value
        if where == 3:
            args[2] = 0
        assert ctx.lib.rn_mesh_place_quadric(ctx._h, *args, _stream()) == _lib.RN_OK, (where, value)
    assert ctx.lib.rn_mesh_place_quadric(ctx._h, *good, _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert np.array_equal(h.bits(out.cpu().numpy()), h.bits(want[0]))
    assert counts.tolist() == want[1].tolist()
    # the context method: what it returns, and tensors that are not what the kernels read
    got, tally = ctx.mesh_place_quadric(v, f, c, p, cell)
    assert got.dtype == torch.float32 and tuple(got.shape) == (nvo, 3)
    assert np.array_equal(h.bits(got.cpu().numpy()), h.bits(want[0]))
    assert tally.dtype == np.int64 and tally.tolist() == want[1].tolist()
    again, _ = ctx.mesh_place_quadric(v, f, c, p, cell, 2.0 ** -10, 1.0, workspace=work, out=out)
    assert again is out and np.array_equal(h.bits(out.cpu().numpy()), h.bits(want[0]))
    assert ctx.mesh_place_quadric_workspace_bytes(nv, nf, nvo) == need
    for bad, match in [
            (dict(vertices=v.double()), "vertices"), (dict(vertices=v.cpu()), "vertices"),
            (dict(faces=f.long()), "faces"), (dict(cluster=c.long()), "cluster"),
            (dict(cluster=c[:-1]), "cluster"), (dict(positions=p.double()), "positions"),
            (dict(positions=p.reshape(-1)), "positions"),
            (dict(positions=torch.zeros((nv + 1, 3), device="cuda")), "positions"),
            (dict(cell=(1.0, 2.0)), "cell"), (dict(workspace=work[:need - 8]), "workspace"),
            (dict(workspace=work[4:]), "workspace"), (dict(out=out[:-1]), "out")]:
        kw = dict(vertices=v, faces=f, cluster=c, positions=p, cell=cell)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ctx.mesh_place_quadric(**kw)
    with pytest.raises(_lib.RaynetHipError, match="rn_mesh_place_quadric"):
        ctx.mesh_place_quadric(v, f, c, p, cell, regularization=2.0)
    # the wrapper: the two GPU calls one after the other, and its ValueErrors with a GPU too
    placed, placed_faces, source, stats = simplify_mesh(vertices, faces, 0.4, placement="quadric",
                                                       return_stats=True)
    assert np.array_equal(h.bits(placed), h.bits(want[0]))
    assert stats["moved"] == want[1][0] and stats["fell_back"] == want[1][1]
    plain = simplify_mesh(vertices, faces, 0.4)
    assert np.array_equal(h.bits(plain[0]), h.bits(positions)) and np.array_equal(plain[1], placed_faces)
    assert np.array_equal(plain[2], source)
    for kw, match in [(dict(placement="median"), "placement"),
                      (dict(placement="quadric", regularization=0.0), "regularization"),
                      (dict(placement="quadric", max_move=nan), "max_move")]:
        with pytest.raises(ValueError, match=match):
            simplify_mesh(vertices, faces, 0.4, **kw)


# ------------------------------------------------------------------------------ e. the chain
def test_from_the_maps_of_two_spheres_to_a_mesh_placed_by_quadrics(tmp_path, capsys):
    """Section 23's scene through fuse_depth_maps --gt --keep_largest 1 --simplify 2, in this
    process, and with --simplify_placement quadric, from the command line: the same faces and as
    many vertices, other bits, and the printed line is the arrays'."""
    from raynet_amd.scripts import fuse_depth_maps
    from raynet_amd.volume import SurfaceMesh
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED)
    scene_dir, preds = str(tmp_path / "scene"), str(tmp_path / "predictions")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    os.makedirs(preds)
    common = ["--gt", "--truncation", "0.25", "--start_end", "0,3", "--grid_shape", "18,22,14",
              "--keep_largest", "1", "--simplify", "2"]
    mean_ply, quadric_ply = str(tmp_path / "mean.ply"), str(tmp_path / "quadric.ply")
    assert fuse_depth_maps.main([scene_dir, preds, mean_ply] + common) == 0
    printed = capsys.readouterr().out
    assert "simplify:" in printed and "placement:" not in printed
    r = subprocess.run([sys.executable, "-m", "raynet_amd.scripts.fuse_depth_maps", scene_dir, preds,
                        quadric_ply] + common + ["--simplify_placement", "quadric"],
                       env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    mean, got = SurfaceMesh.load_ply(mean_ply), SurfaceMesh.load_ply(quadric_ply)
    assert np.array_equal(got.faces, mean.faces) and len(got.vertices) == len(mean.vertices)
    differ = (h.bits(got.vertices) != h.bits(mean.vertices)).any(1)
    assert differ.any() and np.isfinite(got.vertices).all()
    simplify_line = [l for l in printed.splitlines() if l.startswith("simplify:")]
    assert simplify_line and simplify_line[0] in r.stdout.splitlines()
    m = re.search(r"^placement: quadric, (\d+) of (\d+) vertices moved, (\d+) fell back, farthest "
                  r"move (\d+\.\d{3}) cell sides$", r.stdout, re.M)
    assert m is not None, r.stdout
    cell = 2.0 * 2.0 / np.array(grid, D)
    moved = (np.abs(got.vertices.astype(D) - mean.vertices.astype(D)) / cell).max()
    assert [int(m.group(1)), int(m.group(2))] == [int(differ.sum()), len(got.vertices)]
    assert m.group(4) == "%.3f" % moved and 0.0 < moved <= 1.0 + 1e-6
    assert r.stdout.index("simplify:") < r.stdout.index("placement:")
    print(m.group(0))
