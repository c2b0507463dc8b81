"""The iso-surface on the GPU: rn_isosurface_count / rn_isosurface_emit
against tests/isosurface_truth.py -- the same vertices and the same faces, bit for bit and in
order -- the grid-level scan at a size where each of its levels spans more than one workgroup,
the rows beyond the totals, the entries' refusals, and the chain from a forward pass to a mesh
file, a ray caster, a sampled cloud and the metrics."""
import ctypes
import os

import numpy as np
import pytest

import isosurface_truth as it

pytestmark = pytest.mark.gpu

F = np.float32
BBOX = (-0.8, -0.6, -0.4, 0.8, 0.65, 0.41)       # voxel sizes that are no fp32 numbers
PAD = 5


def _context(grid, bbox=BBOX):
    from raynet_amd.common.scene import get_voxel_grid
    from raynet_amd.hip_implementations.context import HipContext
    ctx = HipContext(8, 2, 2, 1, 1, 1, 0, bbox, grid)
    vg = get_voxel_grid(np.array(bbox, F), grid)
    ctx.set_voxel_grid(np.ascontiguousarray(vg.transpose(1, 2, 3, 0)))
    return ctx, [vg[0, :, 0, 0].copy(), vg[1, 0, :, 0].copy(), vg[2, 0, 0, :].copy()]


def _count(ctx, belief, iso, closed):
    """-> (nv, nf, workspace) of rn_isosurface_count."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    size = ctx.lib.rn_isosurface_workspace_bytes(ctx._h, closed)
    assert size > 0 and size % 8 == 0
    work = torch.empty((size,), dtype=torch.uint8, device="cuda")
    totals = (ctypes.c_int64 * 2)(-1, -1)
    ctx._check(ctx.lib.rn_isosurface_count(ctx._h, _ptr(belief), float(iso), closed, _ptr(work),
                                           totals, _stream()))
    return int(totals[0]), int(totals[1]), work


def _extract(ctx, belief, iso, closed):
    """The two entries, with outputs PAD rows longer than the totals and prefilled: ->
    (vertices [nv, 3], faces [nf, 3]) after checking that the PAD rows kept their prefill."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    dev = torch.from_numpy(np.ascontiguousarray(belief, F)).cuda()
    nv, nf, work = _count(ctx, dev, iso, closed)
    assert nv >= 0 and nf >= 0
    vertices = torch.full((nv + PAD, 3), -7.0, dtype=torch.float32, device="cuda")
    faces = torch.full((nf + PAD, 3), -7, dtype=torch.int32, device="cuda")
    ctx._check(ctx.lib.rn_isosurface_emit(ctx._h, _ptr(dev), float(iso), closed, _ptr(work),
                                          nv, nf, _ptr(vertices), _ptr(faces), _stream()))
    v, f = vertices.cpu().numpy(), faces.cpu().numpy()
    assert (v[nv:] == -7).all() and (f[nf:] == -7).all(), "written beyond the totals"
    return v[:nv], f[:nf]


def _assert_same(got, want, what=""):
    (v, f), (tv, tf) = got, want
    assert v.shape == tv.shape and f.shape == tf.shape, (what, v.shape, tv.shape, f.shape, tf.shape)
    assert np.array_equal(f, tf), what
    assert np.array_equal(v.view(np.int32), tv.view(np.int32)), \
        (what, np.abs(v.astype(np.float64) - tv).max() if len(v) else 0)


CASES = {
    # name: (belief, closed, iso, nothing comes out)
    "ball": (it.logistic_ball, 1, 0.5, False),
    "cut ball": (it.cut_ball, 1, 0.5, False),
    "cut ball, open": (it.cut_ball, 0, 0.5, False),
    "noise": (it.noise, 1, 0.5, False),
    "noise, open": (it.noise, 0, 0.5, False),
    "planted voxel": (it.planted_voxel, 1, 0.5, False),
    "all above": (lambda: np.full((3, 4, 5), 0.9, F), 1, 0.5, False),
    "one voxel": (lambda: np.full((1, 1, 1), 0.9, F), 1, 0.5, False),
    "all below": (lambda: np.full((4, 5, 6), 0.2, F), 1, 0.5, True),
    "all below, open": (lambda: np.full((4, 5, 6), 0.2, F), 0, 0.5, True),
    "all above, open": (lambda: np.full((4, 5, 6), 0.9, F), 0, 0.5, True),
    "single layer x, open": (lambda: it.logistic_ball((1, 11, 10), (0, 5, 5)), 0, 0.5, True),
    "single layer z, open": (lambda: it.logistic_ball((12, 11, 1), (5, 5, 0)), 0, 0.5, True),
}


# ------------------------------------------------------------------------------ a. parity
@pytest.mark.parametrize("name", list(CASES))
def test_mesh_is_the_restatement_bit_for_bit(name):
    make, closed, iso, empty = CASES[name]
    belief = make()
    ctx, axes = _context(belief.shape)
    want = it.extract(belief, iso, closed, axes, BBOX)
    assert (len(want[1]) == 0) == empty
    got = _extract(ctx, belief, iso, closed)
    print("%s: %d vertices, %d faces" % (name, len(got[0]), len(got[1])))
    _assert_same(got, want, name)
    if name == "ball":
        # 14 * 13 * 12 lattice points: nine workgroups, the last wavefront partial
        assert (belief.shape, len(got[0]), len(got[1])) == ((12, 11, 10), 756, 1508)
    if name == "all above":
        assert it.is_closed_and_oriented(*got) and it.euler_characteristic(*got) == 2
    if empty:
        # emit is a no-op with both totals 0, whatever the output pointers are
        import torch
        from raynet_amd.hip_implementations.context import _ptr, _stream
        dev = torch.from_numpy(belief).cuda()
        nv, nf, work = _count(ctx, dev, iso, closed)
        assert (nv, nf) == (0, 0)
        assert ctx.lib.rn_isosurface_emit(ctx._h, _ptr(dev), float(iso), closed, _ptr(work), 0, 0,
                                          None, None, _stream()) == 0
    # the wrapper gives the same arrays
    v, f = ctx.isosurface(__import__("torch").from_numpy(belief).cuda(), iso, bool(closed))
    _assert_same((v.cpu().numpy(), f.cpu().numpy()), want, name + " (HipContext.isosurface)")


# ------------------------------------------------------------------- b. every level of the scan
def test_two_balls_over_every_level_of_the_scan():
    """42^3 = 74,088 lattice points: 290 workgroups of 256, whose sums take 2 workgroups, whose
    sums take one -- each level of the scan but the last spans more than one workgroup."""
    belief = it.two_balls()
    assert belief.shape == (40, 40, 40)
    ctx, axes = _context(belief.shape)
    want = it.extract(belief, 0.5, 1, axes, BBOX)
    got = _extract(ctx, belief, 0.5, 1)
    print("two balls: %d vertices, %d faces" % (len(got[0]), len(got[1])))
    _assert_same(got, want, "two balls")
    v, f = got
    E, two, repeated, _ = it.edge_census(f)
    assert E == two and repeated == 0 and 3 * len(f) == 2 * E
    assert len(np.unique(f.ravel())) == len(v)
    assert it.euler_characteristic(v, f) == 4               # two spheres
    assert it.signed_volume(v, f) > 0


# ------------------------------------------------------------------ c. rows beyond the totals
def test_nothing_is_written_beyond_the_rows_asked_for():
    """_extract checks the PAD rows behind nv and nf in every test of this file; here emit is
    also given FEWER rows than the count found: the rows it is given are the first rows of the
    mesh, and nothing behind them is touched."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    belief = it.logistic_ball()
    ctx, axes = _context(belief.shape)
    tv, tf = it.extract(belief, 0.5, 1, axes, BBOX)
    dev = torch.from_numpy(belief).cuda()
    nv, nf, work = _count(ctx, dev, 0.5, 1)
    assert (nv, nf) == (len(tv), len(tf))
    part_v, part_f = nv - 131, nf - 77
    vertices = torch.full((nv + PAD, 3), -7.0, dtype=torch.float32, device="cuda")
    faces = torch.full((nf + PAD, 3), -7, dtype=torch.int32, device="cuda")
    ctx._check(ctx.lib.rn_isosurface_emit(ctx._h, _ptr(dev), 0.5, 1, _ptr(work), part_v, part_f,
                                          _ptr(vertices), _ptr(faces), _stream()))
    v, f = vertices.cpu().numpy(), faces.cpu().numpy()
    assert (v[part_v:] == -7).all() and (f[part_f:] == -7).all()
    assert np.array_equal(v[:part_v].view(np.int32), tv[:part_v].view(np.int32))
    assert np.array_equal(f[:part_f], tf[:part_f])


# ------------------------------------------------------------------------ d. bad arguments
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import HipContext, _ptr, _stream
    belief = torch.from_numpy(it.logistic_ball()).cuda()
    ctx, _ = _context(tuple(belief.shape))
    nv, nf, work = _count(ctx, belief, 0.5, 1)
    filled = work.clone()
    count, emit, last = ctx.lib.rn_isosurface_count, ctx.lib.rn_isosurface_emit, ctx.lib.rn_last_error
    totals = (ctypes.c_int64 * 2)(-1, -1)
    null = ctypes.c_void_p(0)
    INVALID = -1
    for args in [(null, 0.5, 1, _ptr(work), totals), (_ptr(belief), 0.5, 1, null, totals),
                 (_ptr(belief), 0.5, 1, _ptr(work), None), (_ptr(belief), 0.5, 2, _ptr(work), totals),
                 (_ptr(belief), 0.5, -1, _ptr(work), totals),
                 (_ptr(belief), float("nan"), 1, _ptr(work), totals),
                 (_ptr(belief), float("inf"), 0, _ptr(work), totals),
                 (_ptr(belief), 0.0, 1, _ptr(work), totals),
                 (_ptr(belief), -0.5, 1, _ptr(work), totals),
                 (_ptr(belief), 0.5, 1, ctypes.c_void_p(work.data_ptr() + 4), totals)]:
        assert count(ctx._h, *args, _stream()) == INVALID, args
        assert b"rn_isosurface_count" in last(ctx._h)
    assert tuple(totals) == (-1, -1)
    vertices = torch.full((nv, 3), -7.0, dtype=torch.float32, device="cuda")
    faces = torch.full((nf, 3), -7, dtype=torch.int32, device="cuda")
    out = (_ptr(vertices), _ptr(faces))
    for args in [(null, 0.5, 1, _ptr(work), nv, nf) + out, (_ptr(belief), 0.5, 1, null, nv, nf) + out,
                 (_ptr(belief), 0.5, 1, _ptr(work), nv, nf, null, out[1]),
                 (_ptr(belief), 0.5, 1, _ptr(work), nv, nf, out[0], null),
                 (_ptr(belief), 0.5, 3, _ptr(work), nv, nf) + out,
                 (_ptr(belief), float("nan"), 1, _ptr(work), nv, nf) + out,
                 (_ptr(belief), 0.0, 1, _ptr(work), nv, nf) + out,
                 (_ptr(belief), 0.5, 1, _ptr(work), -1, nf) + out,
                 (_ptr(belief), 0.5, 1, _ptr(work), nv, -1) + out,
                 (_ptr(belief), 0.5, 1, _ptr(work), 7 * 2184 + 1, nf) + out]:
        assert emit(ctx._h, *args, _stream()) == INVALID, args
        assert b"rn_isosurface_emit" in last(ctx._h)
    assert ctx.lib.rn_isosurface_workspace_bytes(ctx._h, 2) == -1
    torch.cuda.synchronize()
    assert (vertices == -7).all() and (faces == -7).all() and torch.equal(work, filled)
    # an open lattice takes an iso value that is not positive: everything is inside, no surface
    totals = (ctypes.c_int64 * 2)(-1, -1)
    assert count(ctx._h, _ptr(belief), -0.5, 0, _ptr(work), totals, _stream()) == _lib.RN_OK
    assert tuple(totals) == (0, 0)
    # a context without a voxel grid has no coordinates to give
    bare = HipContext(8, 2, 2, 1, 1, 1, 0, BBOX, tuple(belief.shape))
    with pytest.raises(_lib.RaynetHipError, match="rn_set_voxel_grid"):
        bare.isosurface(belief, 0.5, True)


# ------------------------------------------------------------------------------ e. the chain
def test_from_a_forward_pass_to_a_mesh_a_cloud_and_the_metrics(tmp_path):
    from conftest import GOLDEN
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.common.mesh_io import (get_triangles, parse_gt_data_from_ply,
                                           parse_stl_file_to_pointcloud)
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.mesh import MeshRaycaster
    from raynet_amd.pointcloud import Pointcloud
    from raynet_amd.scripts import compute_metrics, render_volume
    from raynet_amd.synthetic import make_synthetic_scene
    from raynet_amd.volume import SurfaceMesh
    from training_tree import write_plane_scene
    H, W, grid = 20, 30, (18, 22, 14)
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=3, focal=1.5 * H)
    gp = GenerationParameters(depth_planes=16, neighbors=2, grid_shape=np.array(grid, np.int32),
                              max_number_of_marched_voxels=96, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    list(fp.forward_pass(scene, (0, 3, 1)))
    volume = fp.occupancy_volume()
    belief = volume.belief.cpu().numpy()
    print("belief: min %.4g max %.4g, %d of %d voxels >= 0.5"
          % (belief.min(), belief.max(), (belief >= 0.5).sum(), belief.size))
    # 1 - 3: the mesh is closed, oriented, and within the box grown by a voxel
    mesh = volume.mesh()
    assert isinstance(mesh, SurfaceMesh) and not mesh.empty
    print("mesh: %d vertices, %d faces" % (len(mesh.vertices), len(mesh.faces)))
    assert it.is_closed_and_oriented(mesh.vertices, mesh.faces)
    assert it.signed_volume(mesh.vertices, mesh.faces) > 0
    bbox = volume.bbox.astype(np.float64)
    h = (bbox[3:] - bbox[:3]) / np.array(grid)
    assert (mesh.vertices >= bbox[:3] - h).all() and (mesh.vertices <= bbox[3:] + h).all()
    # ... and it is the definition's
    from raynet_amd.common.scene import get_voxel_grid
    vg = get_voxel_grid(volume.bbox, grid)
    want = it.extract(belief, 0.5, True, [vg[0, :, 0, 0], vg[1, 0, :, 0], vg[2, 0, 0, :]],
                      volume.bbox)
    _assert_same((mesh.vertices, mesh.faces), want, "forward pass")
    # 4: file -> mesh_io -> ray caster
    path = str(tmp_path / "surface.ply")
    mesh.save_ply(path)
    points, _, faces = parse_gt_data_from_ply(path)
    assert np.array_equal(points.view(np.int32), mesh.vertices.view(np.int32))
    assert np.array_equal(faces, mesh.faces)
    caster = MeshRaycaster(get_triangles(points, faces))
    assert caster.n_triangles == len(mesh.faces) and caster.area > 0
    # 5: the sampled cloud lies on the surface
    cloud = mesh.pointcloud(2000)
    assert isinstance(cloud, Pointcloud) and np.asarray(cloud.points).shape == (3, 2000)
    dist, _, _ = caster.closest_points(np.asarray(cloud.points).T)
    extent = float(np.abs(bbox).max())
    assert float(dist.max()) <= 1e-5 * extent
    # 6: the command line writes both files, and the metrics take the cloud
    occupancy = str(tmp_path / "occupancy.npz")
    volume.save(occupancy)
    scene_dir, out = str(tmp_path / "scene"), str(tmp_path / "out")
    write_plane_scene(scene_dir, GOLDEN, H=45, W=80, views=3)
    mesh_file, cloud_file = str(tmp_path / "cli_mesh.ply"), str(tmp_path / "cli_cloud.ply")
    assert render_volume.main([scene_dir, occupancy, out, "--start_end", "0,0", "--mesh", mesh_file,
                               "--mesh_cloud", cloud_file, "--mesh_samples", "2000"]) == 0
    assert os.listdir(out) == []                       # no frame asked for, no map written
    cli = SurfaceMesh.load_ply(mesh_file)
    _assert_same((cli.vertices, cli.faces), want, "render_volume --mesh")
    cli_points = parse_stl_file_to_pointcloud(cloud_file)
    assert np.array_equal(cli_points, np.asarray(cloud.points).T)
    args = compute_metrics.build_parser().parse_args(
        [scene_dir, out, "accuracy", "--use_pc_from_depthmap", "--borders", "4"])
    from raynet_amd.common.scene import get_scene
    values, _ = compute_metrics.build_metric("accuracy", args).compute(
        get_scene("restrepo", scene_dir), [0, 1], None,
        Pointcloud(np.ascontiguousarray(cli_points.T)))
    assert np.asarray(values).size == 2000 and np.isfinite(values).all()
