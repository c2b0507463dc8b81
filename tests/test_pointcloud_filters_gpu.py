"""The point-cloud filters on the GPU (raynet_amd.metrics.VoxelMask / ReduceDensity,
csrc/raynet_filters.inl): the kept set EQUALS the truth of
tests/thin_truth.py index for index -- no tolerance -- on inputs whose neighbours sit exactly at
distance r across cell borders, on duplicates, under the seeded hash order and explicit orders,
on degenerate clouds, on a back-projected cloud, and on the reference's own outputs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import thin_truth as truth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _kept_columns(X, kept):
    return np.ascontiguousarray(X[:, kept])


def _filter(X, r, **kw):
    from raynet_amd.metrics import ReduceDensity
    f = ReduceDensity(r, **kw)
    return f.filter(X), f


def _assert_equals_truth(X, r, out, order, what=""):
    kept = truth.greedy_cells(X, r, order)
    assert out.dtype == np.float64 and out.shape[0] == 3
    assert out.shape[1] == kept.sum(), (what, out.shape[1], int(kept.sum()))
    assert np.array_equal(out, _kept_columns(X, kept)), what       # bit for bit, original order
    return kept


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 1e6])
def test_lattice_with_every_neighbour_exactly_at_r(shift, capsys):
    """12^3 lattice of spacing r = 0.25 plus one point that puts the grid's origin off the
    lattice: 1729 points, several workgroups, every neighbour at distance exactly r."""
    X = np.hstack([truth.lattice(), [[-0.1], [-0.07], [-0.13]]]) + shift
    assert X.shape == (3, 1729)
    brute = truth.brute_neighbours(X, 0.25)
    assert sum(len(j) for j in brute) == 2 * 3 * 12 * 12 * 11 + 2
    for kw in (dict(seed=0), dict(seed=5), dict(order=truth.random_order(1729, 1)),
               dict(order=truth.x_sorted_order(X))):
        out, f = _filter(X, 0.25, **kw)
        order = f.visiting_order(1729)
        kept = _assert_equals_truth(X, 0.25, out, order, kw)
        assert np.array_equal(kept, truth.greedy_brute(X, 0.25, order))
        assert "Filter out %d out of 1729 points" % (1729 - kept.sum()) in capsys.readouterr().out
        assert 1 <= f.rounds <= truth.parallel_rounds(X, 0.25, order, brute)[1]


# 2 ---------------------------------------------------------------------------------------------
def test_duplicates():
    """Coincident points are at distance 0 of each other: exactly one of each group survives at
    most, the first in the order."""
    X = truth.lattice_with_duplicates()
    n = X.shape[1]
    first = np.arange(n)                      # the original before its duplicate
    last = np.arange(n)[::-1].copy()          # the duplicate before its original
    for order in (truth.random_order(n, 2), first, last):
        out, f = _filter(X, 0.25, order=order)
        _assert_equals_truth(X, 0.25, out, order)
        assert np.unique(out, axis=1).shape[1] == out.shape[1]
    out, f = _filter(X, 0.25, seed=3)
    _assert_equals_truth(X, 0.25, out, f.visiting_order(n))
    # float32 input is widened
    out32, _ = _filter(X.astype(np.float32), 0.25, order=first)
    assert np.array_equal(out32, _filter(X, 0.25, order=first)[0])


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "sheets"])
def test_seeded_hash_order(name):
    make, r, _ = truth.CASES[name]
    X = make()
    n = X.shape[1]
    kept = {}
    for seed in (0, 11):
        out, f = _filter(X, r, seed=seed)
        order = f.visiting_order(n)
        assert np.array_equal(order, truth.hash_order(seed, n))
        kept[seed] = _assert_equals_truth(X, r, out, order, (name, seed))
    assert not np.array_equal(kept[0], kept[11])


# 4 ---------------------------------------------------------------------------------------------
def test_x_sorted_order_terminates_through_long_chains(capsys):
    make, r, _ = truth.CASES["sheets"]
    X = make()
    order = truth.x_sorted_order(X)
    out, f = _filter(X, r, order=order)
    _assert_equals_truth(X, r, out, order)
    _, jacobi = truth.parallel_rounds(X, r, order)
    with capsys.disabled():
        print("\nx-sorted two sheets: %d rounds on the GPU, %d Jacobi rounds on the host"
              % (f.rounds, jacobi))
    # in-place updates can only decide a point sooner than the Jacobi rounds do
    assert jacobi > 100 and 1 <= f.rounds <= jacobi


# 5 ---------------------------------------------------------------------------------------------
def test_degenerate_clouds():
    out, f = _filter(np.zeros((3, 0)), 0.1)
    assert out.shape == (3, 0) and out.dtype == np.float64
    one = np.array([[1.5], [-2.0], [3.25]])
    assert np.array_equal(_filter(one, 0.1)[0], one)
    # 300 identical points: exactly the first in the order
    same = np.tile(np.array([[0.3], [0.1], [-0.7]]), (1, 300))
    for kw in (dict(seed=4), dict(order=truth.random_order(300, 9))):
        out, f = _filter(same, 0.05, **kw)
        assert out.shape == (3, 1)
        kept = truth.greedy_brute(same, 0.05, f.visiting_order(300))
        assert kept.sum() == 1 and kept[f.visiting_order(300)[0]]
    X = truth.uniform_cube(500, seed=77)
    d2 = ((X[:, :, None] - X[:, None, :]) ** 2).sum(0) + 10.0 * np.eye(500)
    # r below the smallest pair distance: everything is kept
    out, _ = _filter(X, 0.5 * np.sqrt(d2.min()))
    assert np.array_equal(out, X)
    # r above the diameter: exactly the first in the order
    out, f = _filter(X, 2.0, seed=6)
    assert np.array_equal(out, X[:, f.visiting_order(500)[:1]])
    # flat in one axis: a single layer of cells
    flat = truth.uniform_cube(3000, seed=78)
    flat[1] = 0.5
    out, f = _filter(flat, 0.04, seed=1)
    _assert_equals_truth(flat, 0.04, out, f.visiting_order(3000))


# 6 ---------------------------------------------------------------------------------------------
def _backprojected_cloud(seed=0, H=125, W=200):
    """(3, 2 H W) float64: two wavy depth maps back-projected by rn_depthmap_points."""
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.synthetic import ring_cameras
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    clouds = []
    for k, cam in enumerate(ring_cameras(2, H, W, arc=np.pi / 8)):
        depth = 2.6 + 0.2 * np.sin(u / 17.0 + k) * np.cos(v / 11.0) + 0.003 * rng.standard_normal((H, W))
        pts = torch.empty((3, H * W), dtype=torch.float64, device="cuda")
        get_context().depthmap_points(
            H, W, torch.from_numpy(np.ascontiguousarray(cam.P_pinv, np.float64)).cuda(),
            torch.from_numpy(np.asarray(cam.center, np.float64).reshape(4).copy()).cuda(),
            torch.from_numpy(depth.astype(np.float32)).cuda(), pts)
        clouds.append(pts)
    return torch.cat(clouds, dim=1).cpu().numpy()


def test_backprojected_cloud_is_thinned_to_a_maximal_independent_set():
    from raynet_amd.pointcloud import Pointcloud
    X = _backprojected_cloud()
    n, r = X.shape[1], 0.06
    assert n == 50000 and np.isfinite(X).all()
    out, f = _filter(X, r, seed=2)
    kept = _assert_equals_truth(X, r, out, f.visiting_order(n))
    assert 100 < kept.sum() < n // 4
    # independent: thinning the output again, in any order, removes nothing
    m = out.shape[1]
    for kw in (dict(seed=9), dict(order=truth.x_sorted_order(out)), dict(order=np.arange(m)[::-1].copy())):
        assert np.array_equal(_filter(out, r, **kw)[0], out)
    # maximal: every removed point has a kept point within r
    removed = X[:, ~kept]
    cloud = Pointcloud(out)
    _, idx = cloud.nearest_neighbors(removed)
    near = out[:, idx.ravel()]
    d = removed - near
    ok = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] <= r * r
    # (the scan works on float32 copies: where its pair fails the float64 test by a rounding,
    # some other kept point must pass it)
    for i in np.nonzero(~ok)[0]:
        e = out - removed[:, i:i + 1]
        assert (e[0] * e[0] + e[1] * e[1] + e[2] * e[2] <= r * r).any(), i
    assert ok.mean() > 0.999


# 7 ---------------------------------------------------------------------------------------------
def test_the_reference_outputs_bit_for_bit(capsys):
    from raynet_amd.metrics import FiltersFactory, ReduceDensity, VoxelMask
    z = np.load(os.path.join(GOLDEN, "ref_filters.npz"))
    X, r = z["points"], float(z["min_dist"])
    for tag in ("", "2"):
        out = ReduceDensity(r, order=z["order" + tag]).filter(X)
        assert out.dtype == np.float64 and np.array_equal(out, z["reduce_density_points" + tag])
    vm = VoxelMask(z["bbox"], z["mask"])
    inside = vm.filter(X)
    assert inside.dtype == np.float64 and np.array_equal(inside, z["voxel_mask_points"])
    assert "Filter out %d out of 3000 points" % (3000 - inside.shape[1]) in capsys.readouterr().out
    # the factory applies them in order: the mask, then the thinning of what is left
    thin = ReduceDensity(r, seed=12)
    both = FiltersFactory([vm, thin]).filter(X)
    keep = truth.voxel_mask_keep(X, z["bbox"], z["mask"])
    Y = X[:, keep]
    kept = truth.greedy_brute(Y, r, truth.hash_order(12, Y.shape[1]))
    assert np.array_equal(both, Y[:, kept])


# 8 ---------------------------------------------------------------------------------------------
def test_voxel_mask_equals_its_numpy_restatement(tmp_path):
    from raynet_amd.metrics import VoxelMask
    rng = np.random.default_rng(31)
    shape = (6, 5, 8)                                   # steps of exactly 0.5 on every axis
    bbox = np.array([[-1.0, -2.0, 0.0, 2.0, 0.5, 4.0]], np.float32)
    lo, hi = bbox[0, :3].astype(np.float64), bbox[0, 3:].astype(np.float64)
    mask = (rng.random(shape) < 0.5).astype(np.uint8)
    mask[-1, :, :] = 1                                  # the clamp's voxels are observable
    mask[:, :, -1] = rng.integers(0, 3, (6, 5))         # values other than 0 / 1 are not kept
    parts = [lo[:, None] - 0.5 + (hi - lo + 1.0)[:, None] * rng.random((3, 2600))]   # in and out
    inside = lambda n: lo[:, None] + (hi - lo)[:, None] * rng.random((3, n))   # noqa: E731
    for axis in range(3):
        for face in (lo[axis], hi[axis]):               # every face; max of axes 0, 2: the clamp
            P = inside(200)
            P[axis] = face
            parts.append(P)
        # voxel borders: the index's argument is an exact half-integer, both parities
        P = inside(400)
        P[axis] = lo[axis] + 0.5 * rng.integers(0, shape[axis] + 1, 400)
        parts.append(P)
    # just outside a face by one ulp, and the corners
    P = inside(10)
    P[0, :5], P[2, 5:] = np.nextafter(hi[0], np.inf), np.nextafter(lo[2], -np.inf)
    parts.append(P)
    parts.append(np.array([[a, b, c] for a in (lo[0], hi[0]) for b in (lo[1], hi[1])
                           for c in (lo[2], hi[2])]).T)
    X = np.ascontiguousarray(np.hstack(parts))
    assert X.shape[1] >= 5000
    keep = truth.voxel_mask_keep(X, bbox, mask)
    assert 0.1 < keep.mean() < 0.6
    # the clamp is exercised: kept points on the max face of an even axis
    assert (keep & (X[0] == hi[0])).any() and (keep & (X[2] == hi[2])).any()
    vm = VoxelMask(bbox, mask, str(tmp_path))
    out = vm.filter(X)
    assert np.array_equal(out, X[:, keep])
    assert np.array_equal(vm.filter(X.astype(np.float32)),
                          X.astype(np.float32).astype(np.float64)[:, truth.voxel_mask_keep(
                              X.astype(np.float32).astype(np.float64), bbox, mask)])
    body = open(str(tmp_path / "pc_inside_voxel_mask.ply"), "rb").read().split(b"end_header\n", 1)[1]
    assert len(body) == 12 * truth.voxel_mask_keep(
        X.astype(np.float32).astype(np.float64), bbox, mask).sum()


# 9 ---------------------------------------------------------------------------------------------
def _read_ply_xyz(path):
    header, body = open(path, "rb").read().split(b"end_header\n", 1)
    n = int([ln for ln in header.decode().split("\n") if ln.startswith("element vertex")][0].split()[-1])
    pts = np.frombuffer(body, dtype=np.float32).reshape(-1, 3)
    assert pts.shape[0] == n
    return pts


def test_end_to_end_on_a_restrepo_directory(tmp_path, capsys):
    from test_mesh_closest_gpu import _city, _mesh_scene, _small_cams_scene
    from raynet_amd import metrics
    from raynet_amd.scripts import compute_metrics, convert_to_pointcloud
    s = _small_cams_scene(_mesh_scene(tmp_path, _city(3000)))
    H, W = s.image_shape
    preds = str(tmp_path / "predictions")
    os.makedirs(preds)
    for i in range(3):
        np.save(os.path.join(preds, "depth_%03d.npy" % i),
                s.get_surface().depth_map(s.get_image(i).camera, H, W).cpu().numpy())
    out = str(tmp_path / "out")
    # the unfiltered cloud first, to choose a distance from its extent
    args = convert_to_pointcloud.build_parser().parse_args(
        [str(tmp_path / "scene"), preds, out, "--frame_idxs", "0:3", "--borders", "4"])
    cloud, filtered = convert_to_pointcloud.run(s, args)
    assert filtered is None and os.listdir(out) == ["predicted_pc_s_0.ply"]
    assert np.array_equal(_read_ply_xyz(os.path.join(out, "predicted_pc_s_0.ply")),
                          cloud.T.astype(np.float32))
    n = cloud.shape[1]
    d = float(0.02 * (cloud.max(axis=1) - cloud.min(axis=1)).max())
    kept = truth.greedy_cells(cloud, d, truth.hash_order(4, n))
    assert 1 < kept.sum() < n
    args = convert_to_pointcloud.build_parser().parse_args(
        [str(tmp_path / "scene"), preds, out, "--frame_idxs", "0:3", "--borders", "4",
         "--min_distance", repr(d), "--seed", "4"])
    cloud2, filtered = convert_to_pointcloud.run(s, args)
    assert np.array_equal(cloud2, cloud) and np.array_equal(filtered, cloud[:, kept])
    assert sorted(os.listdir(out)) == ["filtered_predicted_pc_s_0.ply",
                                       "pc_after_density_reduction.ply", "predicted_pc_s_0.ply"]
    for name in ("filtered_predicted_pc_s_0.ply", "pc_after_density_reduction.ply"):
        assert np.array_equal(_read_ply_xyz(os.path.join(out, name)),
                              cloud[:, kept].T.astype(np.float32))
    assert "Filter out %d out of %d points" % (n - kept.sum(), n) in capsys.readouterr().out
    # the metrics score filtered clouds
    margs = compute_metrics.build_parser().parse_args(
        [str(tmp_path / "scene"), preds, "accuracy", "completeness", "surface_accuracy",
         "--frame_idxs", "0:3", "--borders", "4", "--output_directory", str(tmp_path / "scores")])
    ff = metrics.FiltersFactory([metrics.ReduceDensity(d, seed=4)])
    results = compute_metrics.run(s, margs, filter_factory=ff)
    gt = np.asarray(s.get_pointcloud().points, np.float64)
    gt_kept = truth.greedy_cells(gt, d, truth.hash_order(4, gt.shape[1]))
    assert results["accuracy"].shape == (kept.sum(), 1)
    assert results["surface_accuracy"].shape == (kept.sum(), 1)
    assert results["completeness"].shape == (gt_kept.sum(), 1) and gt_kept.sum() < gt.shape[1]
    unfiltered = compute_metrics.run(s, margs)
    assert unfiltered["accuracy"].shape == (n, 1)
    assert unfiltered["completeness"].shape == (gt.shape[1], 1)


# 10 --------------------------------------------------------------------------------------------
def test_memory_stays_flat_and_no_ctypes_pointer_is_kept():
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.metrics import ReduceDensity, VoxelMask
    f = ReduceDensity(0.03, seed=1)
    vm = VoxelMask(np.array([[0, 0, 0, 1, 1, 1]], np.float32), np.ones((4, 4, 4), np.uint8))
    rng = np.random.default_rng(8)
    f.filter(rng.random((3, 50000)))
    vm.filter(rng.random((3, 50000)))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(10):
        out = f.filter(rng.random((3, 50000)))
        assert 1000 < out.shape[1] < 50000
    vm.filter(rng.random((3, 50000)))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    byref_type = type(ctypes.byref(ctypes.c_int()))
    for obj in (f, vm, get_context()):
        for name, value in vars(obj).items():
            assert not isinstance(value, (byref_type, ctypes._Pointer)), (type(obj).__name__, name)
