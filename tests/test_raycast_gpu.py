"""Ground truth from scene meshes on the GPU (raynet_amd/mesh.py, csrc/raynet_mesh.inl): the
BVH ray cast equals the fp32 brute force of tests/raycast_truth.py bit for bit, the BVH is
well formed and deterministic, and the scene / metrics / training consumers run on a scene
that ships only a mesh."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import raycast_truth as truth
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

MOCK = os.path.join(GOLDEN, "restrepo_mock_scene_1")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _assert_equal_hits(points, tri, t_points, t_idx, what):
    tri = tri.cpu().numpy() if isinstance(tri, torch.Tensor) else tri
    points = points.cpu().numpy() if isinstance(points, torch.Tensor) else points
    bad = np.nonzero(tri != t_idx)[0]
    assert len(bad) == 0, "%s: %d rays hit another triangle, e.g. ray %d: %d vs %d" % (
        what, len(bad), bad[0], tri[bad[0]], t_idx[bad[0]])
    hit = t_idx >= 0
    diff = np.nonzero((_bits(points[hit]) != _bits(t_points[hit])).any(axis=1))[0]
    assert len(diff) == 0, "%s: %d hit points differ" % (what, len(diff))


# ---- meshes -------------------------------------------------------------------------------
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


def _adversarial(rng, tri, n_random=1500):
    """Rays through vertices, edges, duplicated / zero-area triangles, axis-parallel along
    faces, from inside, missing the root box, with triangles behind the origin."""
    T = len(tri)
    V = tri.reshape(-1, 3)
    lo, hi = V.min(0), V.max(0)
    ext = float((hi - lo).max())
    mid = (lo + hi) / 2
    O, D = [], []
    # random rays from around the mesh towards random points in it
    o = mid + rng.normal(0, 1, (n_random, 3)) * ext
    O.append(o)
    D.append(lo + rng.uniform(0, 1, (n_random, 3)) * (hi - lo))
    # through shared vertices and edge midpoints
    k = rng.integers(0, T, 300)
    t = tri[k].reshape(-1, 3, 3)
    o = mid + rng.normal(0, 1, (300, 3)) * ext
    O += [o, o, o]
    D += [t[:, 0], (t[:, 0] + t[:, 1]) / 2, (t[:, 1] + t[:, 2]) / 2]
    # axis-parallel rays, origins on a triangle's vertex plane (box faces for the city)
    k = rng.integers(0, T, 300)
    for axis in range(3):
        o = tri[k, 3 * (axis % 3):3 * (axis % 3) + 3].copy()
        o[:, axis] = lo[axis] - 0.5 * ext
        d = o.copy()
        d[:, axis] += 1.0
        O.append(o)
        D.append(d)
    # starting inside (at the centre and around it), triangles behind the origin
    o = np.broadcast_to(mid, (200, 3)) + rng.normal(0, 0.05, (200, 3)) * ext
    O.append(o)
    D.append(o + rng.normal(0, 1, (200, 3)))
    # missing the root box: far away, pointing away
    o = mid + np.array([3.0, 0, 0]) * ext + rng.normal(0, 0.1, (100, 3)) * ext
    O.append(o)
    D.append(o + np.array([1.0, 0.2, 0.1]))
    return np.concatenate(O).astype(F), np.concatenate(D).astype(F)


def _det_straddle():
    """Tiny triangles below z = 0, rays along -z: det = a^2 straddles 1e-6 (a ~ 1e-3)."""
    a = (1e-3 * np.linspace(0.997, 1.003, 61)).astype(F)
    tri, O, D = [], [], []
    for i, s in enumerate(a):
        x = F(0.01 * i)
        tri.append([x, 0, -1, x + s, 0, -1, x, s, -1])
        O.append([x + s / 4, s / 4, 0])
        D.append([x + s / 4, s / 4, -1])
    return np.array(tri, F), np.array(O, F), np.array(D, F)


def _raycaster(tri):
    from raynet_amd.mesh import MeshRaycaster
    return MeshRaycaster(tri)


@pytest.mark.parametrize("mesh", ["soup", "sphere", "heightfield", "city", "det"])
def test_kernel_equals_brute_force_bit_for_bit(mesh):
    rng = np.random.default_rng(11)
    if mesh == "det":
        tri, O, D = _det_straddle()
        soup = _soup(rng, 50) * F(0.001) + F(5)
        tri = np.concatenate([tri, soup])
        O2, D2 = _adversarial(rng, tri, 300)
        O, D = np.concatenate([O, O2]), np.concatenate([D, D2])
    else:
        tri = {"soup": lambda: _soup(rng), "sphere": _sphere,
               "heightfield": lambda: _heightfield(rng), "city": lambda: _city(3000)}[mesh]()
        # duplicated triangles (equal keys: the lower index wins) and zero-area ones
        dup = tri[rng.integers(0, len(tri), 40)]
        degenerate = tri[rng.integers(0, len(tri), 20)].copy()
        degenerate[:, 6:9] = degenerate[:, 3:6]
        tri = np.concatenate([tri, dup, degenerate, dup[:10]])
        O, D = _adversarial(rng, tri)
    rc = _raycaster(tri)
    points, idx = rc.first_intersections(O, D)
    t_points, t_idx = truth.first_hits(O, D, tri)
    assert (t_idx >= 0).sum() > (len(O) // 10 if mesh != "det" else 30)   # the rays hit things
    _assert_equal_hits(points, idx, t_points, t_idx, mesh)
    if mesh == "det":
        det_hits = t_idx[:61] >= 0
        assert det_hits.any() and not det_hits.all()     # both sides of the 1e-6 threshold


def test_bvh_invariants_and_determinism():
    rng = np.random.default_rng(3)
    for tri in (_city(5000), _soup(rng, 1), _soup(rng, 2), _sphere(8, 8)):
        T = len(tri)
        a, b = _raycaster(tri), _raycaster(tri)
        assert torch.equal(a.nodes, b.nodes) and torch.equal(a.leaves, b.leaves)
        assert a.depth == b.depth and 0 < a.depth <= 63
        nodes = a.nodes.cpu().numpy()
        leaves = a.leaves.cpu().numpy()
        leaf_tri = leaves[:, 3].view(np.int32)
        assert sorted(leaf_tri) == list(range(T))           # every triangle in one leaf
        p = tri[leaf_tri].reshape(T, 3, 3)
        assert np.array_equal(leaves[:, 0:3], p[:, 0])
        assert np.array_equal(leaves[:, 4:7], p[:, 1] - p[:, 0])
        assert np.array_equal(leaves[:, 8:11], p[:, 2] - p[:, 0])
        refs = np.concatenate([nodes[:, 3], nodes[:, 11]]).view(np.uint32)
        is_leaf = refs >= 0x80000000
        if T > 1:
            assert sorted(refs[is_leaf] & 0x7fffffff) == list(range(T))
            assert sorted(refs[~is_leaf]) == list(range(1, T - 1))   # all but the root once

        def box_of(ref):
            if ref >= 0x80000000:
                q = p[ref & 0x7fffffff]
                return q.min(0), q.max(0)
            n = nodes[ref]
            return (np.minimum(n[0:3], n[8:11]), np.maximum(n[4:7], n[12:15]))

        depth, todo = {0: 0}, [0]
        while todo:
            i = todo.pop()
            n = nodes[i]
            for off in (0, 8):
                ref = np.array([n[off + 3]], F).view(np.uint32)[0]
                lo, hi = box_of(ref)
                assert (n[off:off + 3] <= lo).all() and (hi <= n[off + 4:off + 7]).all()
                if ref < 0x80000000:
                    depth[int(ref)] = depth[i] + 1
                    todo.append(int(ref))
        assert len(depth) == max(T - 1, 1)
        assert max(depth.values()) + 1 == a.depth


def _mock_cameras():
    from raynet_amd.common.camera import Camera
    from raynet_amd.common.scene import read_krt
    cams = sorted(os.listdir(os.path.join(MOCK, "cams_krt")))
    return [Camera(*read_krt(os.path.join(MOCK, "cams_krt", c))) for c in cams]


def test_full_maps_of_the_mock_cameras_over_a_million_triangle_city():
    tri = _city(1_000_000)
    rc = _raycaster(tri)
    H, W = 720, 1280
    cams = _mock_cameras()
    assert len(cams) == 12
    O, Dst, got = [], [], []
    stride = 521
    for k, cam in enumerate(cams):
        D = rc.depth_map(cam, H, W).cpu().numpy()
        assert D.shape == (H, W) and D.dtype == np.float32
        assert (D > 0).mean() > 0.2
        i = np.arange(k, H * W, stride)
        u, v = i // H, i % H
        o, d = truth.pixel_rays(cam.P_pinv, cam.center, u, v)
        O.append(o)
        Dst.append(d)
        got.append(D[v, u])
    O, Dst, got = np.concatenate(O), np.concatenate(Dst), np.concatenate(got)
    assert len(O) >= 20000
    cand = truth.culled_candidates(O, Dst, tri)
    t_points, t_idx = truth.first_hits(O, Dst, tri, candidates=cand)
    dd = t_points.astype(np.float64) - O.astype(np.float64)       # each ray's own centre
    want = np.where(t_idx >= 0, np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) +
                                        dd[:, 2] * dd[:, 2]), 0.0).astype(F)
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, "%d of %d pixels differ, e.g. %r vs %r" % (
        len(bad), len(got), got[bad[:3]], want[bad[:3]])


def test_pixel_path_against_the_reference_golden():
    """The reference's own per-pixel depths (tests/golden/ref_raycast.npz, made by
    gen_raycast_from_reference.py) through the depth-map kernel: the same pixels hit, depths
    within 1e-5 relative; the only exceptions are pixels whose truth hit lies within 1e-5
    (barycentric) of a triangle edge, where the fp32 pixel ray may fall on either side."""
    from raynet_amd.common.camera import Camera
    from raynet_amd.common.mesh_io import get_triangles, parse_gt_data_from_ply
    g = np.load(os.path.join(GOLDEN, "ref_raycast.npz"))
    pts, _, faces = parse_gt_data_from_ply(os.path.join(GOLDEN, "raycast_city.ply"))
    tri = get_triangles(pts, faces)
    rc = _raycaster(tri)
    H, W = int(g["H"]), int(g["W"])
    edge = 0
    total = 0
    for c in range(len(g["K"])):
        cam = Camera(g["K"][c], g["R"][c], g["t"][c])
        D = rc.depth_map(cam, H, W).cpu().numpy()
        ys, xs, ref = g["ys"][c], g["xs"][c], g["depth"][c]        # NaN: the reference missed
        got = D[ys, xs].astype(np.float64)
        ref_hit = ~np.isnan(ref)
        ok = np.where(ref_hit, np.abs(got - np.nan_to_num(ref)) <= 1e-5 * np.abs(
            np.nan_to_num(ref)), got == 0)
        total += len(ys)
        for k in np.nonzero(~ok)[0]:
            o, d = truth.pixel_rays(cam.P_pinv, cam.center, [xs[k]], [ys[k]])
            assert _near_edge(o[0], d[0], tri, 1e-5), "pixel (%d, %d) of camera %d: %r vs %r" % (
                ys[k], xs[k], c, got[k], ref[k])
            edge += 1
    assert edge <= 0.002 * total, (edge, total)
    # explicit rays: the reference's hit points
    points, idx = rc.first_intersections(g["ray_o"], g["ray_d"])
    hit = ~np.isnan(g["ray_hit"][:, 0])
    assert np.array_equal(idx.cpu().numpy() >= 0, hit)
    assert np.allclose(points.cpu().numpy()[hit], g["ray_hit"][hit], rtol=0, atol=1e-5)


def _near_edge(o, d, tri, margin):
    """Some triangle takes the ray within `margin` of its barycentric boundary (float64)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    r = (d - o) / np.linalg.norm(d - o)
    p0 = tri[:, 0:3].astype(np.float64)
    e1 = tri[:, 3:6] - p0
    e2 = tri[:, 6:9] - p0
    pv = np.cross(r, e2)
    det = (e1 * pv).sum(1)
    with np.errstate(all="ignore"):
        inv = 1 / det
        tv = o - p0
        u = (tv * pv).sum(1) * inv
        q = np.cross(tv, e1)
        v = (q * r).sum(1) * inv
    near = (np.abs(u) < margin) | (np.abs(u - 1) < margin) | (np.abs(v) < margin) | \
           (np.abs(u + v - 1) < margin)
    inside = (u > -margin) & (v > -margin) & (u + v < 1 + margin)
    return bool((near & inside).any())


# ---- a scene that ships only a mesh ---------------------------------------------------------
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


def _write_obj(path, tri):
    with open(path, "w") as f:
        for p in tri.reshape(-1, 3):
            f.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for k in range(len(tri)):
            f.write("f %d//1 %d//1 %d//1\n" % (3 * k + 1, 3 * k + 2, 3 * k + 3))


def _mesh_scene(tmp_path, tri, obj_tri=None, H=72, W=128):
    from PIL import Image as PILImage
    dst = str(tmp_path / "scene")
    os.makedirs(str(tmp_path), exist_ok=True)
    shutil.copytree(MOCK, dst)
    os.makedirs(os.path.join(dst, "imgs"))
    for c in sorted(os.listdir(os.path.join(dst, "cams_krt"))):
        PILImage.fromarray(np.zeros((H, W, 3), np.uint8)).save(
            os.path.join(dst, "imgs", c.replace("_cam.txt", ".png")))
    _write_ply(os.path.join(dst, "gt_mesh.ply"), tri)
    if obj_tri is not None:
        _write_obj(os.path.join(dst, "gt_mesh.obj"), obj_tri)
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


def test_restrepo_scene_with_only_a_mesh(tmp_path):
    from raynet_amd.forward_pass import ForwardPass
    from raynet_amd.metrics import PerPixelMeanDepthError
    from raynet_amd.pointcloud import PointcloudFromDepthMaps
    tri = _city(4000)
    path = _mesh_scene(tmp_path, tri)
    s = _small_cams_scene(path)
    H, W = s.image_shape
    D = s.get_depth_map(0)
    assert D.shape == (H, W) and D.dtype == np.float32
    assert (D > 0).any() and (D == 0).any()
    # the map equals the brute force at every pixel
    cam = s.get_image(0).camera
    i = np.arange(H * W)
    o, d = truth.pixel_rays(cam.P_pinv, cam.center, i // H, i % H)
    tp, ti = truth.first_hits(o, d, tri)
    want = np.where(ti >= 0, truth.depths(tp, ti, cam.center), 0).astype(F)
    assert np.array_equal(_bits(D[i % H, i // H]), _bits(want))
    # per pixel: a float where the ray hits, None where it misses
    y, x = np.argwhere(D > 0)[0]
    dp = s.get_depth_for_pixel(0, int(y), int(x))
    assert isinstance(dp, float) and F(dp) == D[y, x]
    y, x = np.argwhere(D == 0)[0]
    assert s.get_depth_for_pixel(0, int(y), int(x)) is None
    pc = s.get_pointcloud()
    assert pc.points.shape == (3, 3 * len(tri)) and np.array_equal(pc.points.T, tri.reshape(-1, 3))
    lo, hi = D[D > 0].min(), D.max()
    assert s.gt_depth_range == (lo, hi)
    # consumers: the metric, the point cloud from depth maps, the ray filter
    pred = [s.get_depth_map(f) * F(1.01) for f in (0, 1)]
    err, _ = PerPixelMeanDepthError(borders=4).compute(s, [0, 1], pred, None)
    assert err.shape == (2,) and np.all(err > 0) and np.all(np.isfinite(err))
    cloud = PointcloudFromDepthMaps(s, [0, 1], pred, borders=4)
    assert cloud.points.shape[0] == 3 and cloud.points.shape[1] > 0
    fp = ForwardPass.__new__(ForwardPass)
    fp._filter_out_rays = True
    rays = fp.get_valid_rays_per_image(s, 0)
    assert len(rays) == int((D != 0).sum())
    assert np.all(D[rays % H, rays // H] != 0)


def test_obj_takes_precedence_and_the_cli_round_trip(tmp_path):
    from raynet_amd.common.scene import RestrepoScene
    city = _city(2000)
    ground = city[:2]
    path = _mesh_scene(tmp_path, city, obj_tri=ground)
    s = _small_cams_scene(path)
    D = s.get_depth_map(0)
    cam = s.get_image(0).camera
    H, W = s.image_shape
    i = np.arange(H * W)
    o, d = truth.pixel_rays(cam.P_pinv, cam.center, i // H, i % H)
    tp, ti = truth.first_hits(o, d, ground)
    assert set(np.unique(ti)) <= {-1, 0, 1}
    want = np.where(ti >= 0, truth.depths(tp, ti, cam.center), 0).astype(F)
    assert np.array_equal(D[i % H, i // H], want)
    # the CLI writes the maps the loader then reads back (full-size images and cameras)
    path = _mesh_scene(tmp_path / "cli", city, H=720, W=1280)
    env = dict(os.environ, PYTHONPATH=REPO)
    subprocess.check_call([sys.executable, "-m", "raynet_amd.scripts.gt_depth_maps", path,
                           "--frames", "0,3"], env=env, cwd=REPO, timeout=300)
    assert sorted(os.listdir(os.path.join(path, "gt"))) == ["gt_depth_0.npy", "gt_depth_3.npy"]
    s2 = RestrepoScene(path)
    fresh = RestrepoScene(path)
    fresh._get_raycaster()
    for f in (0, 3):
        assert s2.get_depthmap_file(f) is not None
        m = s2.get_depth_map(f)
        im = fresh.get_image(f)
        assert np.array_equal(m, fresh._raycaster.depth_map(im.camera, im.height, im.width)
                              .cpu().numpy())
        assert (m > 0).any()


def test_target_points_for_rays(tmp_path):
    from raynet_amd.train_network.raynet_batch_provider import target_points_for_rays
    tri = _city(3000)
    s = _small_cams_scene(_mesh_scene(tmp_path, tri))
    H, W = s.image_shape
    rng = np.random.default_rng(2)
    ridx = rng.integers(0, H * W, 600)
    pts, valid = target_points_for_rays(s, 2, ridx)
    assert pts.shape == (600, 3) and pts.dtype == np.float32 and valid.dtype == bool
    assert valid.any() and not valid.all()
    D = s.get_depth_map(2)
    u, v = ridx // H, ridx % H
    cam = s.get_image(2).camera
    bbox = s.bbox.reshape(6)
    for k in range(600):
        dp = s.get_depth_for_pixel(2, int(v[k]), int(u[k]))
        if dp is None or dp == 0:
            assert not valid[k]
            continue
        # the reference formula: point_from_depth(centre, project(P_pinv, (x, y, 1)) - centre, d)
        ray = np.dot(cam.P_pinv.astype(F), np.array([[u[k]], [v[k]], [1]], F))
        ray = ray / ray[-1]
        a = ray[:3] - cam.center[:3]
        p = (a / np.sqrt(np.sum(a ** 2)) * F(dp) + cam.center[:3]).ravel()
        inside = np.all(p >= bbox[:3]) and np.all(p <= bbox[3:])
        # (the city's ground lies ON the bbox's floor: there the fp32 rounding of the projection
        # -- a matrix product here, one per ray there -- decides, either answer is the rule's)
        on_face = np.abs(np.concatenate([p - bbox[:3], p - bbox[3:]])).min() <= 1e-5
        assert valid[k] == inside or on_face
        if valid[k]:
            assert np.allclose(pts[k], p, rtol=1e-6, atol=1e-6)
            # the point is on the mesh: its distance to the centre is the depth
            assert abs(np.linalg.norm(pts[k] - cam.center[:3].ravel()) - dp) <= 1e-4 * dp
            assert abs(D[v[k], u[k]] - dp) <= 1e-6 * dp
