"""Accuracy and completeness against the ground-truth SURFACE (raynet_amd/mesh.py:
closest_points, sample_surface; metrics.SurfaceAccuracy / SurfaceCompleteness;
scripts/compute_metrics.py): the BVH's nearest-surface query equals the float64 brute force of
tests/surface_truth.py, the sampler is area-weighted, stratified and restatable from its
documented hash, and a cloud that lies ON the mesh scores ~0 where the vertex-based metric
scores a fraction of the scene's extent."""
import os
import shutil

import numpy as np
import pytest
import torch

import surface_truth as truth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MOCK = os.path.join(GOLDEN, "restrepo_mock_scene_1")
F = np.float32


# ---- meshes (the generators of tests/test_raycast_gpu.py) -------------------------------------
def _soup(rng, n=600):
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.normal(0, 0.15, (n, 3, 3))).reshape(n, 9).astype(F)


def _sphere(n_lat=24, n_lon=48, r=1.0):
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, n_lon + 1)
    P = np.stack([r * np.sin(th)[:, None] * np.cos(ph)[None], r * np.sin(th)[:, None] *
                  np.sin(ph)[None], r * np.cos(th)[:, None] * np.ones_like(ph)[None]], -1)
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = P[i, j], P[i + 1, j], P[i + 1, j + 1], P[i, j + 1]
            tris += [np.concatenate([a, b, c]), np.concatenate([a, c, d])]
    return np.array(tris, F)           # (the poles' triangles have zero area)


def _heightfield(rng, n=30):
    x, y = np.meshgrid(np.linspace(-2, 2, n), np.linspace(-2, 2, n), indexing="ij")
    z = 0.3 * np.sin(2 * x) * np.cos(3 * y) + rng.normal(0, 0.02, x.shape)
    P = np.stack([x, y, z], -1)
    tris = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = P[i, j], P[i + 1, j], P[i + 1, j + 1], P[i, j + 1]
            tris += [np.concatenate([a, b, c]), np.concatenate([a, c, d])]
    return np.array(tris, F)


def _city(n):
    from raynet_amd.synthetic import make_box_city
    return make_box_city(n, seed=n)


def _with_duplicates_and_degenerates(rng, tri):
    """+ 40 duplicated triangles, 20 collapsed to a segment (p2 = p1), 10 collapsed to a point,
    in the middle of the list and at its end."""
    dup = tri[rng.integers(0, len(tri), 40)]
    seg = tri[rng.integers(0, len(tri), 20)].copy()
    seg[:, 6:9] = seg[:, 3:6]
    pt = tri[rng.integers(0, len(tri), 10)].copy()
    pt[:, 3:6] = pt[:, 0:3]
    pt[:, 6:9] = pt[:, 0:3]
    # (moved off the mesh, so that they ARE the nearest thing to the queries around them)
    seg += F(0.05) * rng.normal(0, 1, (20, 1)).astype(F).repeat(9, 1)
    pt += F(0.05) * rng.normal(0, 1, (10, 1)).astype(F).repeat(9, 1)
    h = len(tri) // 2
    return np.concatenate([tri[:h], seg[:10], pt[:5], dup, tri[h:], seg[10:], pt[5:], dup[:10]])


def _raycaster(tri):
    from raynet_amd.mesh import MeshRaycaster
    return MeshRaycaster(tri)


def _surface(rc):
    return truth.leaf_vertices(rc.leaves.cpu().numpy())


def _queries(rng, a, b, c, n_random=1000, n_each=100):
    """~2000 queries: random points in 3x the box; vertices, edge midpoints and centroids
    themselves; the box's centre (a sphere's: every triangle near-equidistant); points exactly
    in a triangle's plane but outside it (a city wall's plane, beside the wall); points next to
    the zero-area triangles; points 1e3 extents away."""
    V = np.concatenate([a, b, c])
    lo, hi = V.min(0), V.max(0)
    ext = float((hi - lo).max())
    mid = (lo + hi) / 2
    T = len(a)
    k = rng.integers(0, T, n_each)
    zero = np.nonzero((np.cross(b - a, c - a) == 0).all(1))[0]
    kz = zero[rng.integers(0, len(zero), n_each)] if len(zero) else k
    bary = rng.dirichlet([1, 1, 1], n_each)
    Q = [mid + rng.uniform(-1.5, 1.5, (n_random, 3)) * (hi - lo),
         a[k], b[k], c[k], (a[k] + b[k]) / 2, (b[k] + c[k]) / 2, (a[k] + b[k] + c[k]) / 3,
         bary[:, :1] * a[k] + bary[:, 1:2] * b[k] + bary[:, 2:] * c[k],
         mid[None], np.zeros((1, 3)),
         a[k] + 2.0 * (b[k] - a[k]), a[k] - 0.5 * (b[k] - a[k]) - 0.75 * (c[k] - a[k]),
         a[kz] + rng.normal(0, 0.02 * ext, (n_each, 3)), c[kz],
         mid + rng.normal(0, 1, (n_each, 3)) * 1e3 * ext]
    return np.concatenate(Q), ext


def _check_closest(rc, Q, ext, what, chunk=256):
    a, b, c = _surface(rc)
    dist, closest, tri = rc.closest_points(Q)
    assert dist.dtype == torch.float64 and closest.dtype == torch.float64
    assert tri.dtype == torch.int32 and dist.is_cuda and closest.is_cuda and tri.is_cuda
    assert dist.shape == (len(Q),) and closest.shape == (len(Q), 3) and tri.shape == (len(Q),)
    dist, closest, tri = dist.cpu().numpy(), closest.cpu().numpy(), tri.cpu().numpy()
    assert not np.isnan(dist).any() and not np.isnan(closest).any()
    assert (tri >= 0).all() and (tri < len(a)).all()
    want, _ = truth.brute_force_culled(Q, a, b, c, chunk=chunk)
    bound = 1e-9 * (ext + np.sqrt((Q * Q).sum(1)))
    err = np.abs(dist - want)
    print("%s: %d queries, %d triangles, depth %d: max |dist - truth| = %.3g, the bound's "
          "smallest value %.3g" % (what, len(Q), len(a), rc.depth, err.max(), bound.min()))
    assert (err <= bound).all(), (what, np.argmax(err - bound), err.max())
    # closest lies on the returned triangle and is at distance `dist`
    on = truth.dist_ericson(closest, a[tri], b[tri], c[tri])
    assert (on <= bound).all(), (what, on.max())
    e = Q - closest
    assert (np.abs(np.sqrt((e * e).sum(1)) - dist) <= bound).all()
    # the returned triangle attains the minimum (indices themselves are not compared)
    of_tri = truth.dist_ericson(Q, a[tri], b[tri], c[tri])
    assert (np.abs(of_tri - want) <= bound).all(), (what, np.abs(of_tri - want).max())
    return dist


@pytest.mark.parametrize("mesh", ["soup", "sphere", "heightfield", "city"])
def test_closest_points_equal_the_brute_force(mesh):
    rng = np.random.default_rng(17)
    tri = {"soup": lambda: _soup(rng), "sphere": _sphere,
           "heightfield": lambda: _heightfield(rng), "city": lambda: _city(3000)}[mesh]()
    tri = _with_duplicates_and_degenerates(rng, tri)
    rc = _raycaster(tri)
    a, b, c = _surface(rc)
    Q, ext = _queries(rng, a, b, c)
    assert 1900 <= len(Q) <= 2500
    dist = _check_closest(rc, Q, ext, mesh)
    assert (dist[1000:1700] <= 1e-9 * ext).all()               # the surface's own points
    # host / device, other float dtypes: the same answer for the same float64 values
    Q32 = Q[:300].astype(F)
    d1 = rc.closest_points(Q32)[0]
    d2 = rc.closest_points(torch.from_numpy(Q32).cuda())[0]
    d3 = rc.closest_points(Q32.astype(np.float64))[0]
    assert torch.equal(d1, d2) and torch.equal(d1, d3)
    with pytest.raises(ValueError):
        rc.closest_points(np.zeros((4, 2)))
    assert rc.closest_points(np.zeros((0, 3)))[0].shape == (0,)


def test_closest_points_one_and_two_triangles():
    rng = np.random.default_rng(2)
    for n in (1, 2):
        tri = _soup(rng, n)
        rc = _raycaster(tri)
        Q = rng.uniform(-3, 3, (200, 3))
        _check_closest(rc, Q, 1.0, "%d triangles" % n)


def test_closest_points_in_a_deep_tree():
    rng = np.random.default_rng(23)
    tri = _city(20000)
    rc = _raycaster(tri)
    assert rc.depth > 15                                        # the stack path is exercised
    a, b, c = _surface(rc)
    Q, ext = _queries(rng, a, b, c, n_random=500, n_each=42)
    Q = Q[:1000]
    assert len(Q) == 1000
    _check_closest(rc, Q, ext, "city of 20000", chunk=64)


def test_surface_samples():
    rng = np.random.default_rng(29)
    tri = _with_duplicates_and_degenerates(rng, _city(3000))
    tri = np.concatenate([tri, _sphere(6, 8) * F(0.3) + F(2.0)])        # (pole triangles)
    T = len(tri)
    rc = _raycaster(tri)
    area = truth.areas(tri)
    assert (area == 0).sum() >= 30
    cdf = rc.area_cdf
    assert cdf.dtype == torch.float64 and cdf.is_cuda and cdf.shape == (T,)
    cdf = cdf.cpu().numpy()
    want_cdf = np.cumsum(area)
    assert (np.abs(cdf - want_cdf) <= 1e-12 * want_cdf[-1]).all()
    assert rc.area == cdf[-1]
    a, b, c = truth.file_vertices(tri)
    ext = float((np.concatenate([a, b, c]).max(0) - np.concatenate([a, b, c]).min(0)).max())
    for n in (20011, 7, 1):
        pts, idx = rc.sample_surface(n, seed=3)
        assert pts.dtype == torch.float32 and pts.shape == (n, 3) and pts.is_cuda
        assert idx.dtype == torch.int32 and idx.shape == (n,)
        p, t = pts.cpu().numpy(), idx.cpu().numpy()
        assert (t >= 0).all() and (t < T).all()
        # every sample lies on its triangle
        on = truth.dist_ericson(p.astype(np.float64), a[t], b[t], c[t])
        assert (on <= 1e-6 * ext).all(), on.max()
        # stratified and area-weighted; zero-area triangles get none
        count = np.bincount(t, minlength=T)
        assert (np.abs(count - n * area / want_cdf[-1]) < 2).all()
        assert (count[area == 0] == 0).all()
        # deterministic; another seed, other points
        pts2, idx2 = rc.sample_surface(n, seed=3)
        assert torch.equal(pts.view(torch.int32), pts2.view(torch.int32)) and torch.equal(idx, idx2)
        assert not torch.equal(pts, rc.sample_surface(n, seed=4)[0])
        # the documented hash and formulas, restated in NumPy from the device's own running sum
        rp, rt = truth.sample_surface(tri, cdf, n, 3)
        assert np.array_equal(rt, t)
        assert (np.abs(rp - p) <= np.spacing(np.abs(rp))).all()
    assert rc.sample_surface(0)[0].shape == (0, 3)
    # the default seed is 0
    assert torch.equal(rc.sample_surface(50)[0], rc.sample_surface(50, seed=0)[0])
    with pytest.raises(ValueError):
        _raycaster(tri[area == 0][:5]).sample_surface(10)


# ---- a scene that ships only a mesh: the point of the feature ---------------------------------
def _write_ply(path, tri):
    V = tri.reshape(-1, 3)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment synthetic city\nelement vertex %d\n"
                "property float x\nproperty float y\nproperty float z\nelement face %d\n"
                "property list uchar int vertex_indices\nend_header\n" % (len(V), len(tri)))
        for p in V:
            f.write("%r %r %r\n" % tuple(float(x) for x in p))
        for k in range(len(tri)):
            f.write("3 %d %d %d\n" % (3 * k, 3 * k + 1, 3 * k + 2))


def _mesh_scene(tmp_path, tri, H=72, W=128):
    from PIL import Image as PILImage
    dst = str(tmp_path / "scene")
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copytree(MOCK, dst)
    os.makedirs(os.path.join(dst, "imgs"))
    for c in sorted(os.listdir(os.path.join(dst, "cams_krt"))):
        PILImage.fromarray(np.zeros((H, W, 3), np.uint8)).save(
            os.path.join(dst, "imgs", c.replace("_cam.txt", ".png")))
    if tri is not None:
        _write_ply(os.path.join(dst, "gt_mesh.ply"), tri)
    return dst


def _small_cams_scene(path):
    """The mock cameras see the city at 1280 x 720; the test images are 128 x 72: scale K."""
    from raynet_amd.common.scene import RestrepoScene
    s = RestrepoScene(path)
    for i in range(s.n_images):
        cam = s.get_image(i).camera
        cam._K = cam.K.copy()
        cam._K[:2] *= F(0.1)
        cam._P = cam._P_pinv = cam._center = None
    return s


def test_a_cloud_on_the_mesh_scores_zero_against_the_surface(tmp_path, capsys):
    """The bound is derived, not observed; the test prints the observed
    maximum before it asserts."""
    from raynet_amd.scripts import compute_metrics
    tri = _city(3000)
    ext = float((tri.reshape(-1, 3).max(0) - tri.reshape(-1, 3).min(0)).max())
    s = _small_cams_scene(_mesh_scene(tmp_path, tri))
    H, W = s.image_shape
    surface = s.get_surface()
    assert surface is s._get_raycaster() and surface.n_triangles == len(tri)
    preds = str(tmp_path / "predictions")
    os.makedirs(preds)
    for i in range(s.n_images):
        D = surface.depth_map(s.get_image(i).camera, H, W).cpu().numpy()
        assert (D > 0).any()
        np.save(os.path.join(preds, "depth_%03d.npy" % i), D)
    out = str(tmp_path / "out")
    args = compute_metrics.build_parser().parse_args(
        [str(tmp_path / "scene"), preds, "surface_accuracy", "accuracy", "surface_completeness",
         "--borders", "4", "--output_directory", out, "--surface_samples", "20000", "--seed", "5"])
    results = compute_metrics.run(s, args)
    printed = capsys.readouterr().out
    for name in ("surface_accuracy", "accuracy", "surface_completeness"):
        assert "%s  mean: " % name in printed and " median: " in printed
    assert os.path.getsize(os.path.join(out, "predicted_pc_s_0.ply")) > 1000
    sa, va, sc = results["surface_accuracy"], results["accuracy"], results["surface_completeness"]
    assert sa.shape == va.shape and sa.shape[0] > 10000
    with capsys.disabled():
        print("\nsurface_accuracy of the mesh's own depth maps: max %.3g = %.3g of the extent, "
              "mean %.3g; vertex-based accuracy: mean %.3g; surface_completeness: mean %.3g"
              % (sa.max(), sa.max() / ext, sa.mean(), va.mean(), sc.mean()))
    assert np.isfinite(sa).all()
    assert (sa <= 1e-5 * ext).all(), sa.max() / ext
    assert va.mean() > 100 * sa.mean()
    assert sc.shape == (20000, 1) and np.isfinite(sc).all()
    # --truncate, and the class on its own
    from raynet_amd.metrics import SurfaceAccuracy
    from raynet_amd.pointcloud import Pointcloud
    far = Pointcloud(np.array([[0.0, 100.0], [0.0, 0.0], [50.0, 0.0]]))
    d, pts = SurfaceAccuracy(truncate=7.0).compute(s, [0], None, far)
    assert pts is far.points and np.array_equal(d, [[7.0], [7.0]])
    # a scene without a mesh has no surface
    bare = _small_cams_scene(_mesh_scene(tmp_path / "bare", None))
    with pytest.raises(NotImplementedError):
        bare.get_surface()
