"""Depth-map fusion on the GPU: rn_tsdf_integrate against
tests/fusion_truth.py -- tsdf and weight as int32 views, the same bits, no tolerance (both are
finite by definition, so every bit is comparable) -- over the sizes at which a launch can go
wrong, planted depths and weights, the entries behind the outputs, the entry's refusals, the
sphere of tests/test_fusion_truth.py down to its cleaned mesh, and the chain from a forward pass
to a fused mesh file, its ray caster, the command line and the metrics."""
import ctypes
import os

import numpy as np
import pytest

import fusion_truth as ft
from mesh_harness import PAD, cuda, write_restrepo_scene

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
BBOX = np.array([-1.0, -1.2, -0.9, 1.1, 1.0, 1.3], F)


def _ctx(grid, bbox=BBOX):
    from raynet_amd.fusion import _grid_context
    return _grid_context(bbox, grid)


def _integrate(ctx, V, cameras, H, W, depths, weights, trunc, border):
    """rn_tsdf_integrate on device tensors, with outputs PAD entries longer than G and prefilled
    -> (tsdf, weight) [gx, gy, gz] after checking that the PAD entries kept their prefill."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    G = ctx.G
    tsdf = torch.full((G + PAD,), -7.0, dtype=torch.float32, device="cuda")
    weight = torch.full((G + PAD,), -7.0, dtype=torch.float32, device="cuda")
    ctx._check(ctx.lib.rn_tsdf_integrate(ctx._h, V, _ptr(cameras), H, W, _ptr(depths),
                                         _ptr(weights), float(trunc), float(border), _ptr(tsdf),
                                         _ptr(weight), _stream()))
    t, w = tsdf.cpu().numpy(), weight.cpu().numpy()
    assert (t[G:] == -7).all() and (w[G:] == -7).all(), "written beyond the grid"
    return t[:G].reshape(ctx.grid_shape), w[:G].reshape(ctx.grid_shape)


def _same(got, want, what):
    (t, w), (tt, tw) = got, want
    assert t.shape == tt.shape and w.shape == tw.shape, what
    assert np.isfinite(t).all() and np.isfinite(w).all(), what
    assert np.array_equal(w.view(np.int32), tw.view(np.int32)), \
        (what, "weight", int((w != tw).sum()), np.abs(w.astype(D) - tw).max())
    assert np.array_equal(t.view(np.int32), tt.view(np.int32)), \
        (what, "tsdf", int((t.view(np.int32) != tt.view(np.int32)).sum()),
         np.abs(t.astype(D) - tt).max())


def _scene(V, H, W, seed):
    """V cameras on a ring that see part of the box BBOX, random depths around the box and random
    weights; 5 % of the pixels of either each planted 0 / negative / NaN / +inf."""
    from raynet_amd.common.camera import Camera
    rng = np.random.default_rng(seed)
    cams = []
    for v in range(V):
        a = 2 * np.pi * v / max(V, 1) + 0.1
        cams.append(Camera.look_at([3.5 * np.cos(a), 3.5 * np.sin(a), 0.4 + 0.02 * v], [0, 0, 0],
                                   0.9 * max(H, W), H, W))
    cameras = ft.pack_cameras(cams).reshape(V, 15)
    depths = (3.5 + rng.uniform(-1.5, 1.5, size=(V, H, W))).astype(F)
    weights = rng.uniform(0.05, 4.0, size=(V, H, W)).astype(F)
    for maps in (depths, weights):
        special = rng.random((V, H, W))
        for k, value in enumerate((0.0, -1.0, np.nan, np.inf)):
            maps[(special >= 0.05 * k) & (special < 0.05 * (k + 1))] = value
    return cameras, depths, weights


# ------------------------------------------------------------------------------ a. the sizes
GRIDS = [(1, 1, 1), (3, 4, 5), (7, 5, 67), (24, 22, 20)]


@pytest.mark.parametrize("HW", [(1, 1), (2, 3), (24, 32)])
@pytest.mark.parametrize("V", [0, 1, 2, 5, 33])
@pytest.mark.parametrize("grid", GRIDS)
def test_the_volume_is_the_restatement_bit_for_bit(grid, V, HW):
    """With and without weights, border 0 and 1.5, two truncations."""
    H, W = HW
    ctx = _ctx(grid)
    axes = ft.axes_of(BBOX, grid)
    cameras, depths, weights = _scene(V, H, W, seed=1000 * len(GRIDS) + 100 * V + 10 * H + grid[2])
    d_cameras, d_depths, d_weights = cuda(cameras), cuda(depths), cuda(weights)
    if V == 0:
        d_cameras = d_depths = d_weights = None
    observed = 0
    for use_w in (False, True):
        for border in (0.0, 1.5):
            for trunc in (0.3, 1.7):
                want = ft.integrate(axes, cameras, depths, weights if use_w else None, trunc, border)
                got = _integrate(ctx, V, d_cameras, H, W, d_depths, d_weights if use_w else None,
                                 trunc, border)
                _same(got, want, (grid, V, HW, use_w, border, trunc))
                observed += int((want[1] > 0).sum())
    print("grid %s, V %d, %dx%d: %d voxels observed over the 8 settings" % (grid, V, H, W, observed))
    if V == 0:
        assert observed == 0
    if V >= 2 and HW == (24, 32) and grid[2] >= 20:
        assert observed > 1000           # the scene exercises the sums, not only rejections


# -------------------------------------------------------------------------------- b. the sphere
@pytest.fixture(scope="module")
def sphere():
    s = ft.sphere_scene()
    s["tsdf"], s["weight"] = ft.integrate(s["axes"], s["rows"], s["depths"], None, s["trunc"], 0.0)
    return s


def _same_mesh(mesh, want, what):
    v, f = want
    assert mesh.vertices.shape == v.shape and mesh.faces.shape == f.shape, \
        (what, mesh.vertices.shape, v.shape, mesh.faces.shape, f.shape)
    assert np.array_equal(mesh.faces, f), what
    assert np.array_equal(mesh.vertices.view(np.int32), v.view(np.int32)), what


def test_the_sphere_from_depth_maps_to_the_cleaned_mesh(sphere, tmp_path):
    from raynet_amd.fusion import TSDFVolume, fuse_depth_maps
    s = sphere
    volume = fuse_depth_maps(list(s["depths"]), s["cameras"], s["bbox"], s["grid"], trunc=s["trunc"])
    assert isinstance(volume, TSDFVolume) and volume.trunc == s["trunc"]
    _same((volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy()), (s["tsdf"], s["weight"]),
          "sphere")
    mesh = volume.mesh()
    want = ft.mesh(s["tsdf"], s["weight"], s["axes"], s["bbox"])
    assert len(want[0]) == 2777 and len(want[1]) == 5522
    _same_mesh(mesh, want, "sphere")
    assert np.isfinite(mesh.vertices).all()
    fewer = ft.mesh(s["tsdf"], s["weight"], s["axes"], s["bbox"], min_weight=2.0)
    assert 0 < len(fewer[1]) < len(want[1])
    _same_mesh(volume.mesh(min_weight=2.0), fewer, "sphere, min_weight 2")
    # the default truncation: three of the largest voxel side, from the float32 box
    default = fuse_depth_maps(list(s["depths"]), s["cameras"], s["bbox"], s["grid"])
    side = ((s["bbox"][3:].astype(D) - s["bbox"][:3].astype(D)) / np.array(s["grid"], D)).max()
    assert default.trunc == 3.0 * side and abs(default.trunc - 0.48) < 1e-6
    _same((default.tsdf.cpu().numpy(), default.weight.cpu().numpy()),
          ft.integrate(s["axes"], s["rows"], s["depths"], None, default.trunc, 0.0), "default trunc")
    # the file
    path = str(tmp_path / "sphere.npz")
    volume.save(path)
    _same_mesh(TSDFVolume.load(path).mesh(), want, "sphere, from the file")


def test_no_view_counts_gives_an_empty_mesh(sphere):
    from raynet_amd.fusion import fuse_depth_maps
    s = sphere
    nothing = [np.zeros_like(d) for d in s["depths"]]
    volume = fuse_depth_maps(nothing, s["cameras"], s["bbox"], s["grid"], trunc=s["trunc"])
    assert (volume.tsdf == 1).all() and (volume.weight == 0).all()
    mesh = volume.mesh()
    assert mesh.empty and mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3)


# ----------------------------------------------------------------------------- c. refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    grid = (3, 4, 5)
    ctx = _ctx(grid)
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    cameras, depths, weights = _scene(2, 24, 32, seed=1)
    dcam, ddep, dwei = cuda(cameras), cuda(depths), cuda(weights)
    tsdf = torch.full((ctx.G,), -7.0, dtype=torch.float32, device="cuda")
    weight = torch.full((ctx.G,), -7.0, dtype=torch.float32, device="cuda")
    #       0  1           2   3   4           5           6    7    8           9
    good = [2, _ptr(dcam), 24, 32, _ptr(ddep), _ptr(dwei), 0.3, 1.5, _ptr(tsdf), _ptr(weight)]
    nan, inf = float("nan"), float("inf")
    for at_, value in [(0, -1), (0, 4097), (2, 0), (3, 0), (2, -24), (3, -32), (6, 0.0), (6, -0.3),
                       (6, nan), (6, inf), (7, -1.5), (7, nan), (7, inf), (8, null), (9, null),
                       (1, null), (4, null)]:
        args = list(good)
        args[at_] = value
        assert ctx.lib.rn_tsdf_integrate(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_tsdf_integrate" in last(ctx._h)
    torch.cuda.synchronize()
    assert (tsdf == -7).all() and (weight == -7).all()
    # what is NOT refused: no weights; no views and none of their pointers
    args = list(good)
    args[5] = null
    assert ctx.lib.rn_tsdf_integrate(ctx._h, *args, _stream()) == _lib.RN_OK
    args = [0, null, 24, 32, null, null, 0.3, 1.5, _ptr(tsdf), _ptr(weight)]
    assert ctx.lib.rn_tsdf_integrate(ctx._h, *args, _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert (tsdf == 1).all() and (weight == 0).all()
    # the wrapper: the entry's name on a refusal, and tensors that are not what the kernel reads
    with pytest.raises(_lib.RaynetHipError, match="rn_tsdf_integrate"):
        ctx.tsdf_integrate(dcam, ddep, dwei, -1.0, 0.0)
    got = ctx.tsdf_integrate(dcam, ddep, dwei, 0.3, 0.0)
    assert tuple(got[0].shape) == grid and tuple(got[1].shape) == grid
    for bad, match in [
            (dict(cameras=dcam.float()), "cameras"), (dict(cameras=dcam[:1]), "cameras"),
            (dict(cameras=dcam.t().contiguous().t()), "cameras"),
            (dict(depths=ddep.double()), "depths"), (dict(depths=ddep[:, :, ::2]), "depths"),
            (dict(depths=ddep[0]), "depths"), (dict(depths=ddep.cpu()), "depths"),
            (dict(weights=dwei.half()), "weights"), (dict(weights=dwei[:1]), "weights"),
            (dict(tsdf=tsdf[:-1]), "tsdf"), (dict(tsdf=tsdf.double()), "tsdf"),
            (dict(weight=weight[::2]), "weight"), (dict(weight=weight.int()), "weight")]:
        kw = dict(cameras=dcam, depths=ddep, weights=dwei, trunc=0.3, border=0.0)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ctx.tsdf_integrate(**kw)


# ------------------------------------------------------------------------------ d. the chain
def test_from_a_forward_pass_to_a_fused_mesh_its_file_and_the_metrics(tmp_path):
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.common.mesh_io import parse_gt_data_from_ply, parse_stl_file_to_pointcloud
    from raynet_amd.common.scene import get_scene
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.fusion import TSDFVolume, fuse_scene
    from raynet_amd.pointcloud import Pointcloud
    from raynet_amd.scripts import compute_metrics, fuse_depth_maps
    from raynet_amd.synthetic import make_synthetic_scene
    from raynet_amd.volume import SurfaceMesh
    H, W, grid = 20, 30, (18, 22, 14)
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=3, focal=1.5 * H)
    gp = GenerationParameters(depth_planes=16, neighbors=2, grid_shape=np.array(grid, np.int32),
                              max_number_of_marched_voxels=96, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    # 1: depth maps and their confidence
    pairs = [(np.array(m), np.array(st.confidence))            # (copies: the maps may be leased)
             for m, st in fp.forward_pass(scene, (0, 3, 1), with_statistics=True)]
    maps, conf = [m for m, _ in pairs], [c for _, c in pairs]
    assert len(maps) == 3 and maps[0].shape == (H, W) and conf[0].shape == (H, W)
    # 2: fused with the confidence as weights: the definition's bits
    bbox = np.asarray(scene.bbox, F).reshape(-1)
    volume = fuse_scene(scene, maps, [0, 1, 2], grid, weights=conf)
    cams = [scene.get_image(i).camera for i in range(3)]
    axes = ft.axes_of(bbox, grid)
    want = ft.integrate(axes, ft.pack_cameras(cams), np.stack(maps), np.stack(conf), volume.trunc, 0.0)
    _same((volume.tsdf.cpu().numpy(), volume.weight.cpu().numpy()), want, "forward pass")
    print("fused: %d of %d voxels observed, weight up to %.3g"
          % ((want[1] > 0).sum(), want[1].size, want[1].max()))
    assert (want[1] > 0).sum() > 100
    # 3: the mesh, its file, and back
    mesh = volume.mesh()
    assert isinstance(mesh, SurfaceMesh) and not mesh.empty
    _same_mesh(mesh, ft.mesh(*want, axes, bbox), "forward pass")
    print("mesh: %d vertices, %d faces" % (len(mesh.vertices), len(mesh.faces)))
    path = str(tmp_path / "fused.ply")
    mesh.save_ply(path)
    points, _, faces = parse_gt_data_from_ply(path)
    assert np.array_equal(points.view(np.int32), mesh.vertices.view(np.int32))
    assert np.array_equal(faces, mesh.faces)
    again = SurfaceMesh.load_ply(path)
    _same_mesh(again, (mesh.vertices, mesh.faces), "load_ply")
    # 4: the ray caster over it; sampled points lie on the surface
    caster = mesh.raycaster()
    assert caster.n_triangles == len(mesh.faces) and caster.area > 0
    cloud = mesh.pointcloud(2000)
    assert np.asarray(cloud.points).shape == (3, 2000)
    dist, _, _ = caster.closest_points(np.asarray(cloud.points).T)
    assert float(dist.max()) <= 1e-5 * float(np.abs(bbox).max())
    # 5: the command line, on the scene as a directory (its cameras are the text's float32)
    scene_dir, preds = str(tmp_path / "scene"), str(tmp_path / "predictions")
    gt_maps = []
    for cam in cams:
        d = ft.sphere_depth(cam, H, W, (0.0, 0.0, -0.1), 0.5)
        gt_maps.append(np.where(np.isfinite(d), d, F(0)).astype(F))
    write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    os.makedirs(preds)
    for i in range(3):
        np.save(os.path.join(preds, "depth_%03d.npy" % i), maps[i])
        np.save(os.path.join(preds, "confidence_%03d.npy" % i), conf[i])
    on_disk = get_scene("restrepo", scene_dir)
    common = ["--start_end", "0,3", "--grid_shape", "18,22,14"]
    cli_ply, cli_npz = str(tmp_path / "cli.ply"), str(tmp_path / "cli.npz")
    assert fuse_depth_maps.main([scene_dir, preds, cli_ply, "--confidence_weights",
                                 "--volume", cli_npz] + common) == 0
    same = fuse_scene(on_disk, maps, [0, 1, 2], grid, weights=conf)
    same.mesh().save_ply(str(tmp_path / "api.ply"))
    assert open(cli_ply, "rb").read() == open(str(tmp_path / "api.ply"), "rb").read()
    saved = TSDFVolume.load(cli_npz)
    assert saved.trunc == same.trunc and saved.grid_shape == grid
    _same((saved.tsdf.numpy(), saved.weight.numpy()),
          (same.tsdf.cpu().numpy(), same.weight.cpu().numpy()), "--volume")
    # --min_confidence: the pixels below it weigh nothing
    cut = float(np.median(np.stack(conf)))
    cut_ply = str(tmp_path / "cut.ply")
    assert fuse_depth_maps.main([scene_dir, preds, cut_ply, "--confidence_weights",
                                 "--min_confidence", repr(cut)] + common) == 0
    cut_w = [np.where(c >= F(cut), c, F(0)) for c in conf]
    fuse_scene(on_disk, maps, [0, 1, 2], grid, weights=cut_w).mesh().save_ply(str(tmp_path / "w.ply"))
    assert open(cut_ply, "rb").read() == open(str(tmp_path / "w.ply"), "rb").read()
    assert open(cut_ply, "rb").read() != open(cli_ply, "rb").read()
    # --gt: the scene's ground-truth maps give the ground-truth mesh, here the planted sphere's
    gt_ply, gt_cloud = str(tmp_path / "gt.ply"), str(tmp_path / "gt_cloud.ply")
    assert fuse_depth_maps.main([scene_dir, preds, gt_ply, "--gt", "--truncation", "0.25",
                                 "--normals", "--mesh_cloud", gt_cloud, "--mesh_samples", "2000",
                                 "--seed", "3"] + common) == 0
    gt_mesh = SurfaceMesh.load_ply(gt_ply)
    assert not gt_mesh.empty and gt_mesh.normals is not None and gt_mesh.colors is None
    r = np.sqrt(((gt_mesh.vertices.astype(D) - np.array([0.0, 0.0, -0.1])) ** 2).sum(1))
    cell = (bbox[3:] - bbox[:3]).astype(D) / np.array(grid)
    side = float(cell.max())
    print("--gt: %d vertices, %d faces, distance to the planted sphere max %.3f mean %.3f voxel "
          "sides" % (len(gt_mesh.vertices), len(gt_mesh.faces), np.abs(r - 0.5).max() / side,
                     np.abs(r - 0.5).mean() / side))
    # a vertex lies on a cell's edge or diagonal one end of which some view saw behind the surface
    # it recorded, by at most the truncation (times the factor 1 + trunc / 2z of the sqrt-free
    # distance, z > 2 here)
    assert np.abs(r - 0.5).max() <= 0.25 * (1 + 0.25 / 4) + float(np.sqrt((cell ** 2).sum()))
    # ... and its sampled cloud goes into the accuracy metric
    cli_points = parse_stl_file_to_pointcloud(gt_cloud)
    assert cli_points.shape == (2000, 3)
    args = compute_metrics.build_parser().parse_args(
        [scene_dir, str(tmp_path), "accuracy", "--use_pc_from_depthmap", "--borders", "4"])
    values, _ = compute_metrics.build_metric("accuracy", args).compute(
        on_disk, [0, 1], None, Pointcloud(np.ascontiguousarray(cli_points.T)))
    assert np.asarray(values).size == 2000 and np.isfinite(values).all()
