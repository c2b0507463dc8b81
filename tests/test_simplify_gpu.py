"""Vertex clustering on the GPU: rn_mesh_simplify against
tests/simplify_truth.py -- all five outputs EQUAL the truth's bits, vertices_in and faces_in are
what they were, the rows behind nv_out and nf_out and the bytes behind the workspace keep their
prefill -- over the sizes at which a launch can go wrong: nothing, one vertex, no faces, one
triangle in one cell and in three, a tetrahedron, strips around the wavefront, the workgroup, the
scan tile and two levels of both scans, stars, five thousand vertices in one cell and in five
thousand, a closed and an open iso-surface, anisotropic cells with vertices on their borders,
garbage in the faces and in the positions, three launches that give one result, the entry's
refusals, unique_faces on the device, and the chain from the depth maps of two spheres through the
command line to a simplified, smoothed mesh."""
import ctypes
import os
import re

import numpy as np
import pytest

import components_truth as ct
import isosurface_truth as it
import mesh_harness as h
import simplify_truth as sp
import smooth_truth as st

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
I = np.int32
FILL = -7.5
NO_FACES = np.zeros((0, 3), I)


def _host3(values, ctype):
    plain = int if ctype is ctypes.c_int32 else float
    return (ctype * 3)(*[plain(v) for v in values])


def _launch(vertices, faces, origin, cell, dims):
    """rn_mesh_simplify on device tensors, every output PAD rows longer than its bound and the
    workspace TAIL bytes longer than reported, all prefilled -> (rc, vertices_out, faces_out,
    source, cluster, counts, vertices_in and faces_in on the device, the workspace, the bytes it
    needs)."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    nv, nf = len(vertices), len(faces)
    v, f = h.cuda(np.reshape(vertices, (-1, 3)), F), h.cuda(np.reshape(faces, (-1, 3)), I)
    d = _host3(dims, ctypes.c_int32)
    need = int(ctx.lib.rn_mesh_simplify_workspace_bytes(nv, nf, d))
    cells = int(np.prod(np.asarray(dims, np.int64)))
    assert need >= 32 * cells + 8 * nf + 12 * nv and need % 8 == 0
    work = h.workspace(need)
    vo = h.padded((nv, 3), FILL, torch.float32)
    fo = h.padded((nf, 3), -77, torch.int32)
    so, cl = h.padded(nv, -77, torch.int32), h.padded(nv, -77, torch.int32)
    counts = h.padded(2, -77, torch.int64)
    rc = ctx.lib.rn_mesh_simplify(ctx._h, nv, _ptr(v), nf, _ptr(f), _host3(origin, ctypes.c_double),
                                  _host3(cell, ctypes.c_double), d, _ptr(vo), _ptr(fo), _ptr(so),
                                  _ptr(cl), _ptr(counts), _ptr(work), _stream())
    torch.cuda.synchronize()
    return (rc, vo.cpu().numpy(), fo.cpu().numpy(), so.cpu().numpy(), cl.cpu().numpy(),
            counts.cpu().numpy(), v, f, work, need)


def _same_as_truth(vertices, faces, grid, what, want=None):
    """All five outputs have the truth's bits, the inputs their own, the pads their prefill ->
    the truth's four arrays."""
    from raynet_amd import _lib
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, I).reshape(-1, 3)
    nv = len(vertices)
    origin, cell, dims = grid
    if want is None:
        want = sp.simplify(vertices, faces, origin, cell, dims)
    rc, vo, fo, so, cl, counts, v_after, f_after, work, need = _launch(vertices, faces, origin,
                                                                       cell, dims)
    assert rc == _lib.RN_OK, what
    nvo, nfo = len(want[0]), len(want[1])
    assert counts[:2].tolist() == [nvo, nfo], (what, counts[:2], nvo, nfo)
    h.assert_untouched(counts, 2, -77, (what, "counts"))
    h.assert_untouched(vo, nvo, FILL, (what, "vertices_out"))
    h.assert_untouched(fo, nfo, -77, (what, "faces_out"))
    h.assert_untouched(so, nvo, -77, (what, "source"))
    h.assert_untouched(cl, nv, -77, (what, "cluster"))
    h.assert_untouched(work, need, h.TAIL_BYTE, (what, "the workspace"))
    h.assert_input_kept(v_after, vertices, (what, "vertices_in"))
    h.assert_input_kept(f_after, faces, (what, "faces_in"))
    h.assert_same_bits(vo[:nvo], want[0], what)
    assert np.array_equal(fo[:nfo], want[1]), what
    assert np.array_equal(so[:nvo], want[2]), what
    assert np.array_equal(cl[:nv], want[3]), what
    return want


@pytest.fixture(scope="module")
def ball():
    """The terraced iso-surface of the binary ball through HipContext.isosurface: closed."""
    import torch
    from raynet_amd.fusion import _grid_context
    bbox, _ = it.unit_frame(st.BALL_GRID)
    ctx = _grid_context(bbox, st.BALL_GRID)
    vertices, faces = ctx.isosurface(torch.from_numpy(st.binary_ball_field()).cuda(), 0.5, True)
    vertices, faces = vertices.cpu().numpy(), faces.cpu().numpy()
    assert vertices.shape == (2908, 3) and faces.shape == (5812, 3)
    return vertices, faces


UNIT = (np.zeros(3), np.ones(3), np.array([4, 4, 4], I))


# ------------------------------------------------------------------------------ a. sizes
@pytest.mark.parametrize("nv", [0, 1, 5])
def test_no_faces_leave_no_vertices(nv):
    got = _same_as_truth(st.positions(nv, 1), NO_FACES, UNIT, nv)
    assert len(got[0]) == 0 and (got[3] == -1).all()


def test_one_triangle_in_one_cell_vanishes_and_in_three_survives():
    tri = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.5], [0.25, 0.75, 0.5]], F)
    face = np.array([[0, 1, 2]], I)
    gone = _same_as_truth(tri, face, UNIT, "one cell")
    assert len(gone[0]) == 0 and len(gone[1]) == 0
    kept = _same_as_truth(tri, face, (np.zeros(3), np.full(3, 0.5), np.array([2, 2, 2], I)), "three")
    assert np.array_equal(h.bits(kept[0]), h.bits(tri)) and np.array_equal(kept[1], face)


def test_one_tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    f = ct.tetrahedra(1)[0]
    for cell, dims in ((0.5, 3), (1.0, 2), (4.0, 1)):
        _same_as_truth(v, f, (np.full(3, -0.25), np.full(3, cell), np.full(3, dims, I)), cell)


@pytest.mark.parametrize("permuted", [False, True], ids=["ascending", "permuted"])
@pytest.mark.parametrize("nv", [3, 64, 65, 256, 257, 20003])
def test_strips(nv, permuted):
    """One wavefront, one workgroup, one tile of the scan and two of its levels, for the scan
    over the faces (nv - 2 entries) and the one over the vertices; cells of 0.5, 2 and 7 spacings
    of the strip's vertices along x."""
    vertices, faces = st.strip(nv, seed=nv, permuted=permuted)
    for cell in (0.5, 2.0, 7.0):
        _same_as_truth(vertices, faces, sp.grid_around(vertices, cell), (nv, permuted, cell))


@pytest.mark.parametrize("hub_last", [False, True], ids=["vertex 0", "the last vertex"])
def test_stars(hub_last):
    vertices, faces = st.star(500, seed=5, hub_last=hub_last)
    for cell in (0.5, 2.0):
        _same_as_truth(vertices, faces, sp.grid_around(vertices, cell), (hub_last, cell))


def test_five_thousand_vertices_in_one_cell_and_in_five_thousand():
    """Contention on four words and the mean's exactness; then no contention at all."""
    vertices, faces = sp.one_cell_cloud(5000, seed=2)
    grid = (np.zeros(3), np.ones(3), np.array([8, 8, 8], I))
    assert (sp.cells_of(vertices, *grid)[0] == (3 * 8 + 4) * 8 + 5).all()
    gone = _same_as_truth(vertices, faces, grid, "one cell")
    assert len(gone[0]) == 0
    # two vertices elsewhere keep the cluster in use: its mean is an output
    more = np.concatenate([vertices, np.array([[0.5, 0.5, 0.5], [6.5, 0.5, 0.5]], F)])
    faces = np.concatenate([faces, np.array([[17, 5000, 5001]], I)])
    kept = _same_as_truth(more, faces, grid, "one cell and two")
    assert kept[2].tolist() == [0, 5000, 5001] and kept[1].tolist() == [[0, 1, 2]]
    vertices, faces = sp.spread_cloud(5000, seed=3)
    alone = _same_as_truth(vertices, faces, sp.grid_around(vertices, 1.0), "5000 cells")
    assert np.array_equal(h.bits(alone[0]), h.bits(vertices))


# ------------------------------------------------------------------------------ b. surfaces
@pytest.mark.parametrize("cell", [1.0, 2.0, 4.0])
def test_the_closed_iso_surface_of_the_binary_ball(ball, cell):
    vertices, faces = ball
    got = _same_as_truth(vertices, faces, sp.grid_around(vertices, cell), cell)
    assert 0 < len(got[1]) < len(faces)


@pytest.mark.parametrize("cell", [1.0, 2.0, 4.0])
def test_the_open_iso_surface_of_the_cut_ball(cell):
    vertices, faces = sp.cut_ball_mesh()
    _same_as_truth(vertices, faces, sp.grid_around(vertices, cell), cell)


def test_the_wrapper_and_the_mesh_method_on_the_ball(ball):
    from raynet_amd.simplify import simplify_mesh
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = ball
    want = sp.simplify(vertices, faces, *sp.grid_around(vertices, 2.0))
    want_faces = sp.unique_faces(want[1])[0]
    out, out_faces, source = simplify_mesh(vertices, faces, 2.0)
    assert np.array_equal(h.bits(out), h.bits(want[0])) and np.array_equal(out_faces, want_faces)
    assert np.array_equal(source, want[2])
    assert np.array_equal(simplify_mesh(vertices, faces, 2.0, drop_duplicate_faces=False)[1], want[1])
    rng = np.random.default_rng(4)
    colors = rng.integers(0, 256, size=vertices.shape).astype(np.uint8)
    mesh = SurfaceMesh(vertices, faces, colors=colors)
    mesh.compute_normals()
    small = mesh.simplified(2.0)
    assert np.array_equal(h.bits(small.vertices), h.bits(want[0]))
    assert np.array_equal(small.faces, want_faces) and np.array_equal(small.colors, colors[want[2]])
    assert np.array_equal(h.bits(small.normals),
                          h.bits(SurfaceMesh(want[0], want_faces).compute_normals()))
    assert SurfaceMesh(vertices, faces).simplified(2.0).normals is None
    smooth = small.smoothed(iterations=5)
    assert np.isfinite(smooth.vertices).all() and np.array_equal(smooth.faces, small.faces)


def test_anisotropic_cells_with_vertices_on_their_borders():
    """x in halves, y in three quarters, z 0 or 2: with these cells and origins vertices lie exactly
    on cell borders, in the last cell (q == dims - 1) and on the grid's far face (q == dims: out)."""
    i, j = np.meshgrid(np.arange(9), np.arange(5), indexing="ij")
    v = np.stack([0.5 * i, 0.75 * j - 1.5, np.where((i + j) % 2, 0.0, 2.0)], -1).reshape(-1, 3).astype(F)
    a = (5 * i + j)[:-1, :-1].reshape(-1)
    f = np.concatenate([np.stack([a, a + 5, a + 1], 1), np.stack([a + 1, a + 5, a + 6], 1)]).astype(I)
    for origin, cell, dims in [((0, -1.5, 0), (0.5, 0.75, 2.0), (8, 4, 1)),
                               ((0, -1.5, 0), (1.0, 1.5, 1.0), (4, 2, 2)),
                               ((0.5, -0.75, -2.0), (1.5, 0.75, 2.0), (2, 3, 2)),
                               ((0, -1.5, 0), (1.0, 1.5, 1.0), (5, 3, 3))]:
        grid = (np.array(origin, D), np.array(cell, D), np.array(dims, I))
        c, _, _ = sp.cells_of(v, *grid)
        assert (c >= 0).any() and ((c == -1).any() or dims == (5, 3, 3))
        _same_as_truth(v, f, grid, (origin, cell, dims))


# ------------------------------------------------------------------------------ c. garbage
def test_garbage_in_the_faces_and_the_positions_reads_nothing_out_of_bounds(ball):
    vertices, faces = ball
    grid = sp.grid_around(vertices, 2.0)
    bad_faces, planted = ct.with_garbage(faces, len(vertices), seed=11)
    assert 0.03 < planted.mean() < 0.08
    assert {-1, len(vertices), 2 ** 31 - 1, -2 ** 31} <= set(np.unique(bad_faces[planted]).tolist())
    got = _same_as_truth(vertices, bad_faces, grid, "bad faces")
    assert len(got[1]) < len(sp.simplify(vertices, faces, *grid)[1])
    bad = np.array(vertices, F)
    bad[100, 1], bad[200, 0], bad[300] = np.nan, np.inf, (1e30, -1e30, 3e38)
    got = _same_as_truth(bad, bad_faces, grid, "bad faces and positions")
    # (no operation of the definition makes a NaN that is stored: a singleton keeps its own bits)
    for i in (100, 200, 300):
        if got[3][i] >= 0:
            assert np.array_equal(h.bits(got[0][got[3][i]]), h.bits(bad[i]))
    nothing = np.full_like(vertices, np.nan)
    got = _same_as_truth(nothing, faces, grid, "all NaN")
    assert len(got[0]) == len(vertices) and np.array_equal(got[1], faces)


def test_three_launches_give_one_result():
    vertices, faces = st.strip(20003, seed=9, permuted=True)
    grid = sp.grid_around(vertices, 2.0)
    want = sp.simplify(vertices, faces, *grid)
    for run in range(3):
        _same_as_truth(vertices, faces, grid, run, want)


# ------------------------------------------------------------------------------ d. refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    from raynet_amd.simplify import simplify_mesh
    ctx = h.ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    vertices_np, faces_np = st.strip(40, seed=1, permuted=True)
    nv, nf = 40, len(faces_np)
    grid = sp.grid_around(vertices_np, 2.0)
    v, f = torch.from_numpy(vertices_np).cuda(), torch.from_numpy(faces_np).cuda()
    d = _host3(grid[2], ctypes.c_int32)
    o, c = _host3(grid[0], ctypes.c_double), _host3(grid[1], ctypes.c_double)
    need = int(ctx.lib.rn_mesh_simplify_workspace_bytes(nv, nf, d))
    work = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    vo = torch.full((nv, 3), FILL, dtype=torch.float32, device="cuda")
    fo = torch.full((nf, 3), -77, dtype=torch.int32, device="cuda")
    so = torch.full((nv,), -77, dtype=torch.int32, device="cuda")
    cl = torch.full((nv,), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -77, dtype=torch.int64, device="cuda")

    def at_(p, byte):
        return ctypes.c_void_p(p.value + byte)

    def three(values, k, bad, ctype):
        values = list(values)
        values[k] = bad
        return _host3(values, ctype)

    #       0   1        2   3        4  5  6  7         8         9         10        11
    good = [nv, _ptr(v), nf, _ptr(f), o, c, d, _ptr(vo), _ptr(fo), _ptr(so), _ptr(cl), _ptr(counts),
            _ptr(work)]                                                               # 12
    nan, inf = float("nan"), float("inf")
    cases = [(0, -1), (2, -1), (0, 2 ** 31 - 1), (0, 2 ** 40), (2, (2 ** 31 - 1) // 3 + 1),
             (2, 2 ** 40), (1, null), (3, null), (4, null), (5, null), (6, null), (7, null),
             (8, null), (11, null), (12, null), (12, at_(_ptr(work), 4)), (12, at_(_ptr(work), 1)),
             (7, _ptr(v)), (8, _ptr(f)), (7, _ptr(work)), (8, _ptr(work)),
             (6, _host3((65536, 32768, 1), ctypes.c_int32)),
             (6, _host3((2 ** 31 - 1, 2, 1), ctypes.c_int32))]
    for k in range(3):
        cases += [(6, three(grid[2], k, 0, ctypes.c_int32)), (6, three(grid[2], k, -3, ctypes.c_int32))]
        cases += [(5, three(grid[1], k, x, ctypes.c_double)) for x in (0.0, -1.0, nan, inf)]
        cases += [(4, three(grid[0], k, x, ctypes.c_double)) for x in (nan, inf, -inf)]
    for where, value in cases:
        args = list(good)
        args[where] = value
        assert ctx.lib.rn_mesh_simplify(ctx._h, *args, _stream()) == INVALID, (where, value)
        assert b"rn_mesh_simplify" in last(ctx._h), (where, value)
    assert ctx.lib.rn_mesh_simplify_workspace_bytes(-1, 0, d) == -1
    assert ctx.lib.rn_mesh_simplify_workspace_bytes(0, 2 ** 40, d) == -1
    assert ctx.lib.rn_mesh_simplify_workspace_bytes(2 ** 31 - 1, 0, d) == -1
    assert ctx.lib.rn_mesh_simplify_workspace_bytes(1, 1, _host3((65536, 32768, 1), ctypes.c_int32)) == -1
    torch.cuda.synchronize()
    assert (vo == FILL).all() and (work == 0xA5).all() and (fo == -77).all()
    assert (so == -77).all() and (cl == -77).all() and (counts == -77).all()
    assert np.array_equal(h.bits(v.cpu().numpy()), h.bits(vertices_np))
    # what is NOT refused: no faces and no pointers to them; nothing at all; source and cluster
    # not wanted; the limits of the sizes (the size entry: nothing that large is allocated here)
    assert ctx.lib.rn_mesh_simplify(ctx._h, nv, _ptr(v), 0, null, o, c, d, _ptr(vo), null, _ptr(so),
                                    _ptr(cl), _ptr(counts), _ptr(work), _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0] and (cl == -1).all() and (vo == FILL).all()
    counts.fill_(-77)
    assert ctx.lib.rn_mesh_simplify(ctx._h, 0, null, 0, null, o, c, d, null, null, null, null,
                                    _ptr(counts), null, _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [0, 0]
    want = sp.simplify(vertices_np, faces_np, *grid)
    for where, value in [(9, null), (10, null), (12, at_(_ptr(work), 8)),
                         (5, _host3((5e-324, 1.0, 1.0), ctypes.c_double))]:
        args = list(good)
        args[where] = value
        assert ctx.lib.rn_mesh_simplify(ctx._h, *args, _stream()) == _lib.RN_OK, (where, value)
        torch.cuda.synchronize()
        if where != 5:
            assert counts.tolist() == [len(want[0]), len(want[1])]
            assert np.array_equal(fo.cpu().numpy()[:len(want[1])], want[1])
    assert ctx.lib.rn_mesh_simplify_workspace_bytes(
        2 ** 31 - 2, (2 ** 31 - 1) // 3, _host3((2 ** 31 - 1, 1, 1), ctypes.c_int32)) > 2 ** 36
    # the context method: what it returns, and tensors that are not what the kernels read
    got = ctx.mesh_simplify(v, f, *grid)
    assert [t.dtype for t in got] == [torch.float32, torch.int32, torch.int32, torch.int32]
    assert tuple(got[0].shape) == (len(want[0]), 3) and tuple(got[1].shape) == (len(want[1]), 3)
    assert tuple(got[2].shape) == (len(want[0]),) and tuple(got[3].shape) == (nv,)
    for mine, theirs in zip(got, want):
        assert np.array_equal(mine.cpu().numpy().view(np.uint32), theirs.view(np.uint32))
    again = ctx.mesh_simplify(v, f, *grid, workspace=work)
    assert np.array_equal(again[1].cpu().numpy(), want[1])
    assert ctx.mesh_simplify_workspace_bytes(nv, nf, grid[2]) == need
    for bad, match in [
            (dict(vertices=v.double()), "vertices"), (dict(vertices=v.cpu()), "vertices"),
            (dict(faces=f.long()), "faces"), (dict(dims=(3, 0, 2)), "dims"),
            (dict(dims=(3, 2)), "dims"), (dict(dims=(1.5, 2, 2)), "dims"),
            (dict(origin=(0.0, 1.0)), "origin"), (dict(cell=(1.0, 2.0)), "cell"),
            (dict(workspace=work[:need - 8]), "workspace"), (dict(workspace=work[4:]), "workspace")]:
        kw = dict(vertices=v, faces=f, origin=grid[0], cell=grid[1], dims=grid[2])
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ctx.mesh_simplify(**kw)
    with pytest.raises(_lib.RaynetHipError, match="rn_mesh_simplify"):
        ctx.mesh_simplify(v, f, grid[0], (1.0, -1.0, 1.0), grid[2])
    # the wrapper raises its ValueErrors with a GPU as without one
    for kw, match in [(dict(cell=0.0), "cell"), (dict(cell=1e-5), "cell"),
                      (dict(cell=1.0, origin=(nan, 0.0, 0.0)), "origin"),
                      (dict(cell=1.0, faces=np.array([[0, 1, nv]])), "faces")]:
        args = dict(vertices=vertices_np, faces=faces_np)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            simplify_mesh(**args)


def test_unique_faces_on_the_device_is_the_dictionarys(ball):
    import torch
    from raynet_amd.simplify import unique_faces
    vertices, faces = ball
    sheet = sp.thin_sheet()
    cases = [sp.simplify(vertices, faces, *sp.grid_around(vertices, 6.0))[1],
             sp.simplify(*sheet, *sp.grid_around(sheet[0], 0.5))[1],
             np.concatenate([faces, faces[::-1, [2, 0, 1]]]), NO_FACES,
             np.array([[2 ** 31 - 1, 0, -2 ** 31], [-2 ** 31, 2 ** 31 - 1, 0], [5, 5, 5]], I)]
    for faces in cases:
        want, keep = sp.unique_faces(faces)
        got = unique_faces(torch.from_numpy(np.ascontiguousarray(faces, I)).cuda())
        assert got.is_cuda and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want.reshape(-1, 3))
    assert not sp.unique_faces(cases[1])[1].all() and not sp.unique_faces(cases[2])[1].all()


# ------------------------------------------------------------------------------ e. the chain
def test_from_the_maps_of_two_spheres_to_a_simplified_smoothed_mesh(tmp_path, capsys):
    """Section 23's scene through fuse_depth_maps --gt --keep_largest 1 --simplify 2 --smooth 5
    --normals; the run without --simplify is the yardstick, a run without --smooth either gives
    the mesh both start from."""
    from raynet_amd.common.mesh_io import parse_stl_file_to_pointcloud
    from raynet_amd.common.scene import get_scene
    from raynet_amd.pointcloud import Pointcloud
    from raynet_amd.scripts import compute_metrics, fuse_depth_maps
    from raynet_amd.volume import SurfaceMesh
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED)
    scene_dir, preds = str(tmp_path / "scene"), str(tmp_path / "predictions")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    os.makedirs(preds)
    on_disk = get_scene("restrepo", scene_dir)
    common = ["--gt", "--truncation", "0.25", "--start_end", "0,3", "--grid_shape", "18,22,14",
              "--keep_largest", "1", "--normals"]
    rough_ply, yard_ply = str(tmp_path / "rough.ply"), str(tmp_path / "yardstick.ply")
    small_ply, cloud_ply = str(tmp_path / "small.ply"), str(tmp_path / "small_cloud.ply")
    yard_cloud = str(tmp_path / "yardstick_cloud.ply")
    cloud = ["--mesh_samples", "2000", "--seed", "3"]
    assert fuse_depth_maps.main([scene_dir, preds, rough_ply] + common) == 0
    assert fuse_depth_maps.main([scene_dir, preds, yard_ply, "--smooth", "5", "--mesh_cloud",
                                 yard_cloud] + cloud + common) == 0
    assert "simplify:" not in capsys.readouterr().out
    assert fuse_depth_maps.main([scene_dir, preds, small_ply, "--simplify", "2", "--smooth", "5",
                                 "--mesh_cloud", cloud_ply] + cloud + common) == 0
    printed = capsys.readouterr().out
    rough, yard = SurfaceMesh.load_ply(rough_ply), SurfaceMesh.load_ply(yard_ply)
    got = SurfaceMesh.load_ply(small_ply)
    # the file is the truth applied to the mesh both runs smooth: cells of two voxel sides anchored
    # at the box's minimum, the duplicates dropped, then section 23's smoothing
    voxel = 2.0 / np.array(grid, D)
    cell = 2.0 * voxel
    anchor = np.array([-1.0, -1.0, -1.0])
    anchor = anchor + np.minimum(np.floor((rough.vertices.min(0).astype(D) - anchor) / cell), 0) * cell
    dims = (np.floor((rough.vertices.max(0).astype(D) - anchor) / cell) + 1).astype(I)
    want = sp.simplify(rough.vertices, rough.faces, anchor, cell, dims)
    want_faces = sp.unique_faces(want[1])[0]
    border = st.boundary_vertices(want_faces, len(want[0]))
    smooth = st.smooth(want[0], want_faces, 5, 0.5, -0.53, border, float(voxel.min()))
    assert np.array_equal(got.faces, want_faces)
    assert np.array_equal(h.bits(got.vertices), h.bits(smooth))
    assert got.normals is not None and np.isfinite(got.normals).all()
    # the printed counts are the file's, and the faces are fewer than the yardstick's
    m = re.search(r"^simplify: cell 2 voxel sides, (\d+) -> (\d+) vertices, (\d+) -> (\d+) faces$",
                  printed, re.M)
    assert m is not None, printed
    assert [int(x) for x in m.groups()] == [len(rough.vertices), len(got.vertices),
                                            len(rough.faces), len(got.faces)]
    assert printed.index("simplify:") < printed.index("smooth:")
    assert len(got.faces) < len(yard.faces) and len(yard.faces) == len(rough.faces)
    # the cloud sampled from the result goes through the accuracy metric, like the yardstick's
    args = compute_metrics.build_parser().parse_args(
        [scene_dir, str(tmp_path), "accuracy", "--use_pc_from_depthmap", "--borders", "4"])
    means = []
    for path in (yard_cloud, cloud_ply):
        points = parse_stl_file_to_pointcloud(path)
        assert points.shape == (2000, 3)
        values, _ = compute_metrics.build_metric("accuracy", args).compute(
            on_disk, [0, 1], None, Pointcloud(np.ascontiguousarray(points.T)))
        assert np.asarray(values).size == 2000 and np.isfinite(values).all()
        means.append(float(np.mean(values)))
    print("faces %d -> %d; mean accuracy of 2000 samples: %.5f unsimplified, %.5f simplified"
          % (len(yard.faces), len(got.faces), means[0], means[1]))
