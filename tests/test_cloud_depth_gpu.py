"""Ground-truth depth from a point cloud on the GPU (raynet_amd/cloud_depth.py,
csrc/raynet_cloud.inl): the raw z-buffer equals the NumPy restatement
tests/cloud_truth.py bit for bit, the filtered maps equal the truth's filter on the same buffer,
the maps of a densely sampled mesh agree with its exact ray cast, and a DTU scan that ships only
its point cloud works end to end through DTUScene and the command-line tool."""
import os

import numpy as np
import pytest
import torch

import cloud_truth as truth
from dtu_tree import write_dtu_tree

pytestmark = pytest.mark.gpu

F = np.float32
H0, W0 = 37, 53


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def _cameras():
    """Camera 0: axis-aligned with power-of-two focal and principal point (26.5, 18.5), so that
    pixel coordinates of hand-placed points are exact; cameras 1, 2: general look_at views."""
    from raynet_amd.common.camera import Camera
    K = np.array([[32.0, 0, 26.5], [0, 32.0, 18.5], [0, 0, 1.0]])
    return [Camera(K, np.eye(3), np.zeros((3, 1))),
            Camera.look_at([1.5, -1.0, -2.0], [0, 0, 2.0], 1.0 * H0, H0, W0, up=(0, -1.0, 0)),
            Camera.look_at([-2.0, 0.5, -1.0], [0, 0, 2.5], 1.3 * H0, H0, W0, up=(0, -1.0, 0))]


def _at(us, vs, z):
    """Points that camera 0 projects to exactly (us, vs) at depth z (all exact in fp32)."""
    us, vs = np.asarray(us, np.float64), np.asarray(vs, np.float64)
    z = np.broadcast_to(np.asarray(z, np.float64), us.shape)
    return np.stack([(us - 26.5) / 32.0 * z, (vs - 18.5) / 32.0 * z, z], axis=-1).astype(F)


def _random_cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, 3)) * [2.5, 1.8, 1.5] + [0, 0, 2.5]).astype(F)


def _clouds():
    clouds = {"n=%d" % n: _random_cloud(n, seed=n) for n in (0, 1, 63, 64, 65, 255, 257, 10_007)}
    ks = np.arange(0, 12, dtype=np.float64)               # both parities of k
    clouds["u = k + 0.5"] = _at(ks + 0.5, 3.0 + ks, 2.0)
    clouds["v = k + 0.5"] = _at(5.0 + 2 * ks, ks + 0.5, 4.0)
    clouds["image borders"] = np.concatenate([
        _at([-0.5, W0 - 0.5, -0.5 - 2.0 ** -10, W0 - 0.5 + 2.0 ** -10], [7.0, 8.0, 9.0, 10.0], 2.0),
        _at([7.0, 8.0, 9.0, 10.0], [-0.5, H0 - 0.5, -0.5 - 2.0 ** -10, H0 - 0.5 + 2.0 ** -10], 2.0)])
    behind = _at([10.0, 11.0, 12.0], [5.0, 5.0, 5.0], 2.0)
    behind[0, 2], behind[1, 2] = -2.0, 0.0                # behind the camera, and Xc_2 = 0
    clouds["behind the camera"] = np.concatenate([behind, [[0.0, 0.0, 0.0], [0.1, 0.1, -0.0]]]).astype(F)
    bad = _random_cloud(40, seed=5)
    for i, (axis, value) in enumerate((a, v) for a in range(3) for v in (np.nan, np.inf, -np.inf)):
        bad[3 * i, axis] = value
    bad[30] = [np.nan, np.inf, -np.inf]
    clouds["nan and inf"] = bad
    dup = _random_cloud(50, seed=6)
    clouds["duplicates"] = np.concatenate([dup, dup[::2], dup, _at([20.0] * 4, [9.0] * 4, 2.0)])
    # 20,000 distinct depths on the ray of camera 0's pixel (26, 18): x = y = -z / 64
    z = 1.0 + np.arange(20_000, dtype=np.float64) / 16384.0
    clouds["one pixel"] = _at(np.full(z.shape, 26.0), np.full(z.shape, 18.0),
                              np.random.default_rng(7).permutation(z))
    return clouds


@pytest.fixture(scope="module")
def cameras():
    return _cameras()


@pytest.fixture(scope="module")
def clouds():
    return _clouds()


def _gpu_zbuffer(points, cams, H, W):
    from raynet_amd.cloud_depth import CloudDepthRenderer
    return CloudDepthRenderer(points).zbuffer(cams, H, W).cpu().numpy()


@pytest.mark.parametrize("V", [1, 3])
def test_raw_buffer_is_bit_identical_to_the_truth(cameras, clouds, V):
    cams = cameras[:V]
    rows = truth.camera_rows(cams)
    for name, pts in clouds.items():
        want = truth.zbuffer(pts, rows, H0, W0)
        got = _gpu_zbuffer(pts, cams, H0, W0)
        assert got.shape == (V, H0, W0) and got.dtype == F
        bad = np.argwhere(_bits(got) != _bits(want))
        assert len(bad) == 0, "%s, V = %d: %d pixels differ, e.g. %s: %r vs %r" % (
            name, V, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        if name in ("u = k + 0.5", "v = k + 0.5", "one pixel", "duplicates", "n=10007"):
            assert np.isfinite(want[0]).any(), name        # the case does land in the image
    # what the hand-placed cases are there for, on the truth (the GPU equals it):
    z = truth.zbuffer(clouds["u = k + 0.5"], rows[:1], H0, W0)[0]
    assert sorted(np.nonzero(np.isfinite(z))[1].tolist()) == [0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12]
    z = truth.zbuffer(clouds["image borders"], rows[:1], H0, W0)[0]
    assert np.isfinite(z).sum() == 4 and np.isfinite(z[7, 0]) and np.isfinite(z[8, W0 - 1]) \
        and np.isfinite(z[0, 7]) and np.isfinite(z[H0 - 1, 8])
    z = truth.zbuffer(clouds["behind the camera"], rows[:1], H0, W0)[0]
    assert np.isfinite(z).sum() == 1 and z[5, 12] == 2.0
    z = truth.zbuffer(clouds["one pixel"], rows[:1], H0, W0)[0]
    assert np.isfinite(z).sum() == 1 and z[18, 26] == 1.0


def test_raw_buffer_does_not_depend_on_the_order_of_the_points(cameras):
    pts = _random_cloud(10_007, seed=11)
    perm = np.random.default_rng(12).permutation(len(pts))
    a = _gpu_zbuffer(pts, cameras, H0, W0)
    b = _gpu_zbuffer(pts[perm], cameras, H0, W0)
    assert np.array_equal(_bits(a), _bits(b))
    assert np.isfinite(a).mean() > 0.5


def test_counted_entry_gives_the_same_buffer_and_the_landed_pairs(cameras, clouds):
    from raynet_amd.cloud_depth import CloudDepthRenderer
    rows = truth.camera_rows(cameras)
    for name in ("n=10007", "one pixel", "nan and inf", "n=0"):
        pts = clouds[name]
        r = CloudDepthRenderer(pts)
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        bits = r.zbuffer_bits(rows, H0, W0, counts=counts).cpu().numpy()
        assert np.array_equal(bits, _bits(truth.zbuffer(pts, rows, H0, W0))), name
        landed, skipped = (int(c) for c in counts.cpu())
        assert landed == truth.landed_pairs(pts, rows, H0, W0), name
        # every filled pixel took at least one atomic
        assert 0 <= skipped <= landed - int((bits != 0x7F800000).sum()), name


def test_wrapper_validates_its_arguments(cameras):
    from raynet_amd.cloud_depth import CloudDepthRenderer
    from raynet_amd.hip_implementations import get_context
    with pytest.raises(ValueError):
        CloudDepthRenderer(np.zeros((5, 4), F))
    r = CloudDepthRenderer(_random_cloud(10))
    with pytest.raises(ValueError):
        r.zbuffer(cameras, 0, 5)
    with pytest.raises(ValueError):
        r.depth_maps(cameras, H0, W0, closing_radius=-1)
    ctx = get_context()
    rows = torch.from_numpy(truth.camera_rows(cameras)).cuda()
    zbuf = torch.full((3, H0, W0), 0x7F800000, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ctx.cloud_zbuffer(r.points.double(), rows, H0, W0, zbuf)           # dtype
    with pytest.raises(ValueError):
        ctx.cloud_zbuffer(r.points, rows.float(), H0, W0, zbuf)
    with pytest.raises(ValueError):
        ctx.cloud_zbuffer(r.points, rows, H0, W0 + 1, zbuf)                # zbuf too small
    with pytest.raises(ValueError):
        ctx.cloud_zbuffer(r.points.t(), rows, H0, W0, zbuf)                # strided
    with pytest.raises(ValueError):
        ctx.cloud_zbuffer(r.points, rows, H0, W0, zbuf.float())
    assert (zbuf == 0x7F800000).all()
    assert r.zbuffer([], H0, W0).shape == (0, H0, W0)


# ---- the sampled city: one mesh, its ray cast and its cloud, shared -------------------------
HC, WC = 120, 160


@pytest.fixture(scope="module")
def city():
    """make_box_city(300, seed=3), its exact ray cast in two views and surface samples at a mean
    spacing of 0.8 pixel footprints (the smaller of the two views' footprints; a footprint =
    the median hit distance / the focal length)."""
    from raynet_amd.common.camera import Camera
    from raynet_amd.mesh import MeshRaycaster
    from raynet_amd.synthetic import make_box_city
    rc = MeshRaycaster(make_box_city(300, seed=3))
    focals = [1.0 * HC, 1.1 * HC]
    cams = [Camera.look_at([4, -3, 7], [0, 0, 0.2], focals[0], HC, WC),
            Camera.look_at([7, -6, 5], [0, 0, 0.2], focals[1], HC, WC)]
    D = [rc.depth_map(c, HC, WC).cpu().numpy().astype(np.float64) for c in cams]
    footprints = [float(np.median(d[d > 0])) / f for d, f in zip(D, focals)]
    n = int(np.ceil(rc.area / (0.8 * min(footprints)) ** 2))
    points = rc.sample_surface(n, seed=0)[0]
    return {"cams": cams, "D": D, "footprints": footprints, "points": points,
            "points_host": points.cpu().numpy()}


def _distances(Z, camera):
    """z-depths [H, W] -> distances to the camera centre, 0 kept: z * |K^-1 (u, v, 1)|, what
    DTUScene.get_depth_map computes."""
    H, W = Z.shape
    us, vs = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.einsum("ij,jhw->ihw", np.linalg.inv(np.asarray(camera.K, np.float64)),
                     np.stack([us, vs, np.ones_like(us)]))
    return Z.astype(np.float64) * np.linalg.norm(rays, axis=0)


def _scores(Z, D, camera, footprint):
    """(share of the ray cast's hit pixels that have a depth, gross share of those)."""
    hit = D > 0
    covered = hit & (Z != 0)
    gross = covered & (np.abs(_distances(Z, camera) - D) > 3 * footprint)
    return covered.sum() / float(hit.sum()), gross.sum() / float(max(covered.sum(), 1))


@pytest.mark.parametrize("S", [0, 1, 2])
def test_filtered_maps_equal_the_truths_filter_on_the_gpu_buffer(city, S):
    from raynet_amd.cloud_depth import CloudDepthRenderer
    from raynet_amd.common.camera import Camera
    # every 7th sample at 37 x 53: about one point per pixel, holes and hidden surfaces
    cams = [Camera.look_at([4, -3, 7], [0, 0, 0.2], 1.0 * H0, H0, W0),
            Camera.look_at([7, -6, 5], [0, 0, 0.2], 1.1 * H0, H0, W0),
            Camera.look_at([-6, 2, 2.5], [0, 0, 0.2], 0.9 * H0, H0, W0)]
    rows = truth.camera_rows(cams)
    r = CloudDepthRenderer(city["points"][::7].contiguous())
    z0 = r.zbuffer(cams, H0, W0).cpu().numpy()
    for gain, tau in ((1.5, 1.0), (0.0, 0.5), (2.25, 0.0)):
        got = r.depth_maps(cams, H0, W0, closing_radius=S, slope_gain=gain,
                           tau_px=tau).cpu().numpy()
        keep = truth.filter_keep(z0, rows, S, gain, tau)
        assert np.array_equal(got != 0, keep), (S, gain, tau)
        assert np.array_equal(_bits(got), _bits(np.where(keep, z0, F(0)))), (S, gain, tau)
        filled = np.isfinite(z0)
        assert filled.mean() > 0.3
        if S == 0:
            assert np.array_equal(keep, filled)
        else:
            assert 0 < keep.sum() < filled.sum()                       # the filter does filter


def test_maps_of_a_sampled_mesh_agree_with_its_ray_cast(city):
    """The caps of the fidelity table, on both cameras, for the truth run
    on the GPU-sampled points and for the GPU maps, which must equal it bit for bit.  Measured
    on an MI355X (84470 points): first camera raw coverage 0.883, gross 0.084, filtered 0.780 /
    0.025; second camera 0.903 / 0.049 and 0.832 / 0.012."""
    from raynet_amd.cloud_depth import CloudDepthRenderer
    cams, pts = city["cams"], city["points_host"]
    rows = truth.camera_rows(cams)
    r = CloudDepthRenderer(city["points"])
    raw_gpu = r.depth_maps(cams, HC, WC, closing_radius=0).cpu().numpy()
    out_gpu = r.depth_maps(cams, HC, WC).cpu().numpy()
    raw = truth.depth_maps(pts, rows, HC, WC, closing_radius=0)
    out = truth.depth_maps(pts, rows, HC, WC)
    for k, cam in enumerate(cams):
        cov_raw, gross_raw = _scores(raw[k], city["D"][k], cam, city["footprints"][k])
        cov, gross = _scores(out[k], city["D"][k], cam, city["footprints"][k])
        print("camera %d: %d points, footprint %.5f; raw coverage %.3f gross %.3f; filtered "
              "coverage %.3f gross %.3f" % (k, len(pts), city["footprints"][k], cov_raw, gross_raw,
                                            cov, gross))
        assert cov >= 0.70, "the truth alone misses the coverage cap"
        assert gross <= 0.04, "the truth alone misses the gross cap"
        assert gross <= 0.5 * gross_raw, "the truth alone misses the improvement cap"
    assert np.array_equal(_bits(raw_gpu), _bits(raw))
    assert np.array_equal(_bits(out_gpu), _bits(out))


# ---- end to end: a DTU scan that ships only its point cloud ------------------------------------
def _dtu_cameras(H, W):
    from raynet_amd.common.camera import Camera
    return [Camera.look_at(p, [0, 0, 0.2], 1.0 * H, H, W)
            for p in ([4, -3, 7], [5, -1, 6.5], [3, -5, 6])]


def test_dtu_scan_with_only_a_cloud_works_end_to_end(city, tmp_path, capsys):
    from raynet_amd.common.scene import DTUScene
    from raynet_amd.pointcloud import PointcloudFromDepthMaps
    from raynet_amd.scripts import gt_depth_maps
    H, W = 60, 80
    base = write_dtu_tree(tmp_path, _dtu_cameras(H, W), H, W, scan=1, points=city["points_host"])
    s = DTUScene(base, 1)
    assert s.n_images == 3 and s._depth_map_paths == []
    rendered = []
    for i in range(3):
        Z = s.get_gt_depth_map(i)
        assert Z.shape == (H, W) and Z.dtype == F and (Z != 0).mean() > 0.5
        assert s.get_gt_depth_map(i) is Z                       # kept per frame
        # the fallback is the renderer's map of the loader's own camera, and the truth's
        want = truth.depth_maps(city["points_host"], truth.camera_rows([s.get_image(i).camera]),
                                H, W)[0]
        assert np.array_equal(_bits(Z), _bits(want))
        D = s.get_depth_map(i)
        assert D.shape == (H, W) and D.dtype == F
        assert np.array_equal(D != 0, Z != 0) and (D[Z != 0] >= Z[Z != 0] * (1 - 1e-5)).all()
        rendered.append(Z)
    renderer = s._cloud_renderer
    assert renderer is not None and renderer.n_points == len(city["points_host"])
    assert s._get_cloud_renderer() is renderer                  # built once
    cloud = PointcloudFromDepthMaps(s, [0, 1, 2], [s.get_depth_map(i) for i in range(3)],
                                    borders=4).points
    assert cloud.shape[0] == 3 and cloud.shape[1] == sum(
        int((Z[4:-4, 4:-4] != 0).sum()) for Z in rendered)
    # points built from the ground-truth distances lie on the city: within its bounding box
    # (-5, -5, -0.7, 5, 5, 1.5), give or take the pixel whose centre stands for the point
    assert np.abs(cloud[:2]).max() < 5.3 and cloud[2].min() > -0.9 and cloud[2].max() < 1.7

    assert gt_depth_maps.main([base, "--dataset_type", "dtu", "--scene_idx", "1"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    files = sorted(os.listdir(os.path.join(base, "Depth", "scan001")))
    assert files == ["depth_001.npy", "depth_002.npy", "depth_003.npy"]
    assert lines == ["frame %d: %d of %d pixels filled" % (i, int((rendered[i] != 0).sum()), H * W)
                     for i in range(3)]
    fresh = DTUScene(base, 1)
    for i in range(3):
        assert np.array_equal(_bits(fresh.get_gt_depth_map(i)), _bits(rendered[i]))
        assert np.array_equal(fresh.get_depth_map(i), s.get_depth_map(i))
    assert fresh._cloud_renderer is None


def test_dtu_scan_with_depth_files_never_constructs_a_renderer(city, tmp_path, monkeypatch):
    import raynet_amd.cloud_depth as cloud_depth
    from raynet_amd.common.scene import DTUScene
    H, W = 60, 80
    maps = [np.full((H, W), 6.0 + k, F) for k in range(3)]
    base = write_dtu_tree(tmp_path, _dtu_cameras(H, W), H, W, scan=1,
                          points=city["points_host"][:1000], depth_maps=maps)

    def refuse(*args, **kwargs):
        raise AssertionError("a scan with depth files must not render its cloud")
    monkeypatch.setattr(cloud_depth, "CloudDepthRenderer", refuse)
    s = DTUScene(base, 1)
    for i in range(3):
        assert np.array_equal(s.get_gt_depth_map(i), maps[i])
        assert s.get_depth_map(i).shape == (H, W)
    assert s._cloud_renderer is None
