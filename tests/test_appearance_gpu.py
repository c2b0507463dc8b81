"""Normals and colours on the GPU: rn_vertex_area_normals and
rn_project_colors against tests/appearance_truth.py -- colors and weight as int32 views, the view
masks and the area normals, the same bits, no tolerance -- over the sizes at which a launch can
go wrong, planted points, depths and normals, the rows behind the outputs, the entries' refusals,
and the chain from a forward pass to a coloured mesh file and coloured clouds."""
import ctypes
import os

import numpy as np
import pytest

import appearance_truth as at
import isosurface_truth as it
import mesh_harness as h

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
NS = (0, 1, 63, 64, 65, 257, 300)


def _project(ctx, n, points, normals, cameras, images, depths, tol, min_cos, border, mode,
             H=None, W=None, C=None):
    """rn_project_colors on device tensors, with outputs PAD rows longer than n and prefilled: ->
    (colors [n, C], weight [n], views [n] uint32) after checking that the PAD rows kept their
    prefill."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    V = 0 if cameras is None else len(cameras)
    if images is not None:
        H, W, C = (int(s) for s in images.shape[1:])
    colors = h.padded((n, C), -7.0, torch.float32)
    weight, views = h.padded(n, -7.0, torch.float32), h.padded(n, -7, torch.int32)
    ctx._check(ctx.lib.rn_project_colors(
        ctx._h, n, _ptr(points), _ptr(normals), V, _ptr(cameras), H, W, C, _ptr(images),
        _ptr(depths), float(tol), float(min_cos), float(border), int(mode), _ptr(colors),
        _ptr(weight), _ptr(views), _stream()))
    c, w, m = colors.cpu().numpy(), weight.cpu().numpy(), views.cpu().numpy()
    for out in (c, w, m):
        h.assert_untouched(out, n, -7, "written beyond the rows asked for")
    return c[:n], w[:n], m[:n].view(np.uint32)


def _same(got, want, what):
    (c, w, m), (tc, tw, tm) = got, want
    assert c.shape == tc.shape and w.shape == tw.shape and m.shape == tm.shape, what
    assert np.array_equal(m, tm), (what, "views", int((m != tm).sum()))
    assert np.array_equal(w.view(np.int32), tw.view(np.int32)), \
        (what, "weight", np.abs(w.astype(D) - tw).max())
    assert np.array_equal(c.view(np.int32), tc.view(np.int32)), \
        (what, "colors", np.abs(c.astype(D) - tc).max())


def _scene(V, H, W, C, seed):
    """300 points in [-2, 2]^3 with normals (some zero), V cameras on a ring that see part of
    them, random images, and depth maps that hide some points, with planted 0 / negative / NaN /
    +inf pixels."""
    from raynet_amd.common.camera import Camera
    rng = np.random.default_rng(seed)
    n = NS[-1]
    points = rng.uniform(-2, 2, size=(n, 3)).astype(F)
    normals = rng.normal(size=(n, 3)).astype(F) * rng.choice(np.array([1e-3, 1, 50], F), (n, 1))
    normals[rng.random(n) < 0.1] = 0
    cams = []
    for v in range(V):
        a = 2 * np.pi * v / max(V, 1) + 0.1
        cams.append(Camera.look_at([3.5 * np.cos(a), 3.5 * np.sin(a), 0.4 + 0.05 * v], [0, 0, 0],
                                   0.9 * max(H, W), H, W))
    cameras = at.pack_cameras(cams).reshape(V, 15)
    images = rng.random((V, H, W, C)).astype(F)
    depths = (3.5 + rng.uniform(-1.5, 1.5, size=(V, H, W))).astype(F)
    special = rng.random((V, H, W))
    for k, value in enumerate((0.0, -1.0, np.nan, np.inf)):
        depths[(special >= 0.05 * k) & (special < 0.05 * (k + 1))] = value
    return points, normals, cameras, images, depths


# ------------------------------------------------------------------------------ a. the sizes
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("HW", [(1, 1), (2, 3), (24, 32)])
@pytest.mark.parametrize("V", [0, 1, 2, 5, 32])
def test_colours_are_the_restatement_bit_for_bit(V, HW, C):
    """Every n of NS, both modes, with and without normals and depths, border 0 and 1.5: a
    point's row does not depend on n, so the truth is computed once per setting for the 300
    points and every smaller n is its prefix."""
    H, W = HW
    ctx = h.ctx()
    points, normals, cameras, images, depths = _scene(V, H, W, C, seed=100 * V + 10 * H + C)
    d_points, d_normals = h.cuda(points), h.cuda(normals)
    d_cameras, d_images, d_depths = h.cuda(cameras), h.cuda(images), h.cuda(depths)
    if V == 0:
        d_cameras = d_images = d_depths = None
    counted = 0
    for mode in (0, 1):
        for use_n in (False, True):
            for use_d in (False, True):
                for border in (0.0, 1.5):
                    want = at.project_colors(points, normals if use_n else None, cameras, images,
                                             depths if use_d else None, 0.05, 0.2, border, mode)
                    counted += int((want[2] != 0).sum())
                    for n in NS:
                        got = _project(ctx, n, d_points, d_normals if use_n else None, d_cameras,
                                       d_images, d_depths if use_d else None, 0.05, 0.2, border,
                                       mode, H, W, C)
                        _same(got, tuple(a[:n] for a in want),
                              (V, HW, C, mode, use_n, use_d, border, n))
    print("V %d, %dx%d, C %d: %d rows seen over the 16 settings" % (V, H, W, C, counted))
    if V and HW == (24, 32):
        assert counted > 100         # the scene exercises the colour path, not only rejections
    if V == 0:
        assert counted == 0


def test_blend_and_best_share_weights_and_masks():
    ctx = h.ctx()
    points, normals, cameras, images, depths = _scene(5, 24, 32, 3, seed=7)
    dev = [h.cuda(a) for a in (points, normals, cameras, images, depths)]
    blend = _project(ctx, 300, *dev, 0.05, 0.0, 0.0, 0)
    best = _project(ctx, 300, *dev, 0.05, 0.0, 0.0, 1)
    assert np.array_equal(blend[1].view(np.int32), best[1].view(np.int32))
    assert np.array_equal(blend[2], best[2])
    many = np.array([bin(m).count("1") > 1 for m in blend[2]])
    assert many.any() and not np.array_equal(blend[0][many], best[0][many])
    one = np.array([bin(m).count("1") == 1 for m in blend[2]])
    assert one.any()
    # a single view: the blend is w col / w, the best is col -- equal to rounding
    assert np.abs(blend[0][one].astype(D) - best[0][one]).max() < 1e-6


# ----------------------------------------------------------------------- b. planted inputs
def test_planted_points_depths_normals_and_ties():
    """appearance_truth.planted_scene: points behind the camera, on its plane and at its centre,
    X exactly 0, exactly W - 1 and one fp64 step beyond, X at 0.5 / 1.5 / 2.5 for the half-to-even
    depth lookup, NaN and infinite coordinates, depths 0 / negative / NaN / +inf, normals zero,
    facing away and exactly perpendicular, and two views of exactly equal weight.  The conditions
    are check_planted's, which tests/test_appearance_truth.py holds the truth to."""
    ctx = h.ctx()
    scene = at.planted_scene()
    dev = [h.cuda(scene[k]) for k in ("points", "normals", "cameras", "images", "depths")]
    for mode in (0, 1):
        want = at.project_colors(scene["points"], scene["normals"], scene["cameras"],
                                 scene["images"], scene["depths"], 0.0, 0.0, 0.0, mode)
        got = _project(ctx, len(scene["points"]), *dev, 0.0, 0.0, 0.0, mode)
        _same(got, want, "planted, mode %d" % mode)
        at.check_planted(got, scene, mode)


def test_one_sided_occlusion_with_a_tolerance():
    ctx = h.ctx()
    cams, images, depths = at.plane_scene()
    cameras = at.pack_cameras(cams)
    rng = np.random.default_rng(11)
    pts = np.zeros((257, 3), F)
    pts[:, 0] = rng.uniform(-3.0, 3.0, 257)
    pts[:, 1] = rng.uniform(-2.4, 2.4, 257)
    dev = [h.cuda(a) for a in (cameras, images, depths)]
    for z, tol in ((0.0, 0.1), (0.5, 0.0), (-0.5, 0.1), (-0.05, 0.1)):
        p = pts.copy()
        p[:, 2] = z
        want = at.project_colors(p, None, cameras, images, depths, tol, 0.0, 0.0, 0)
        got = _project(ctx, 257, h.cuda(p), None, *dev, tol, 0.0, 0.0, 0)
        _same(got, want, ("plane", z, tol))
        if z == -0.5:
            assert (got[2] == 0).all()
        else:
            assert (got[2] != 0).sum() > 100
    # the plane's colours come back within the float32 rounding of its images
    want = at.affine_field(pts[:, 0].astype(D), pts[:, 1].astype(D))
    got = _project(ctx, 257, h.cuda(pts), None, *dev, 0.1, 0.0, 0.0, 0)
    seen = got[2] != 0
    assert np.abs(got[0][seen].astype(D) - want[seen]).max() <= 1e-6


# ------------------------------------------------------------------------------- c. normals
def _normals(ctx, vertices, faces, offsets, corners, nv=None, nf=None):
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    nv = len(vertices) if nv is None else nv
    nf = len(faces) if nf is None else nf
    out = h.padded((nv, 3), -7.0, torch.float32)
    # (held in names until the copy back: a tensor nobody holds returns its memory at once)
    dv, df = h.cuda(vertices, F), h.cuda(faces, np.int32)
    do, dc = h.cuda(offsets, np.int32), h.cuda(corners, np.int32)
    ctx._check(ctx.lib.rn_vertex_area_normals(ctx._h, nv, _ptr(dv), nf, _ptr(df), _ptr(do),
                                              _ptr(dc), _ptr(out), _stream()))
    got = out.cpu().numpy()
    del dv, df, do, dc
    h.assert_untouched(got, nv, -7, "written beyond the vertices")
    return got[:nv]


MESHES = {
    "ball": (it.logistic_ball, (756, 1508)),
    "noise": (it.noise, (1024, None)),
    "two balls": (it.two_balls, (8006, None)),
}


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name, (make, _) in MESHES.items():
        belief = make()
        bbox, axes = it.unit_frame(belief.shape)
        out[name] = it.extract(belief, 0.5, True, axes, bbox)
    return out


@pytest.mark.parametrize("name", list(MESHES))
def test_area_normals_are_the_restatement_bit_for_bit(meshes, name):
    import torch
    from raynet_amd.appearance import corner_table, vertex_normals
    v, f = meshes[name]
    nv, nf = MESHES[name][1]
    assert len(v) == nv and (nf is None or len(f) == nf)
    offsets, corners = at.corner_table(f, len(v))
    # the package's table (one stable sort, a bincount, a cumsum) is the definition's
    d_off, d_cor = corner_table(torch.from_numpy(f).cuda(), len(v))
    assert np.array_equal(d_off.cpu().numpy(), offsets) and np.array_equal(d_cor.cpu().numpy(), corners)
    want = at.area_normals(v, f)
    got = _normals(h.ctx(), v, f, offsets, corners)
    valence = at.valence(f, len(v))
    print("%s: %d vertices, %d faces, valence %d..%d, %d zero normals"
          % (name, len(v), len(f), valence.min(), valence.max(), (want == 0).all(1).sum()))
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if name == "two balls":
        assert valence.max() == 10 and len(v) > 31 * 256         # more than one workgroup
    if name == "noise":
        zero = (want == 0).all(1)
        assert zero.any() and np.array_equal(got[zero].view(np.int32) & 0x7fffffff,
                                             np.zeros((zero.sum(), 3), np.int32))
    # the public function: the same vectors, and their unit form
    area = vertex_normals(v, f, unit=False)
    assert np.array_equal(area.view(np.int32), want.view(np.int32))
    unit = vertex_normals(v, f, unit=True)
    length = np.sqrt((unit.astype(D) ** 2).sum(1))
    zero = (want == 0).all(1)
    assert np.abs(length[~zero] - 1).max() < 1e-6 and (unit[zero] == 0).all()


def test_unused_vertices_and_bad_indices_are_skipped_and_harm_nothing():
    ctx = h.ctx()
    v, f = at.tetrahedron()
    v5 = np.concatenate([v, [[9, 9, 9]]]).astype(F)
    offsets, corners = at.corner_table(f, 5)
    want = at.area_normals(v5, f)
    got = _normals(ctx, v5, f, offsets, corners)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and (got[4] == 0).all()
    assert np.array_equal(got[:4], 4 * v)
    # a mesh without faces: rows of zeros (faces and corners are never read)
    got = _normals(ctx, v5, np.zeros((0, 3), np.int32), np.zeros(6, np.int32),
                   np.zeros(0, np.int32))
    assert (got == 0).all()
    # a hand-made table with corners beyond 3 nf and below 0, offsets that run beyond the table
    # and backwards, and a face that names a vertex beyond nv: those are skipped (a guard on the
    # reads: every index that IS used lies inside the arrays), the rest is as it was
    bad_corners = corners.copy()
    bad_corners[[1, 4]] = [99, -3]
    bad_offsets = offsets.copy()
    bad_offsets[4:] = [1 << 30, -5]                 # vertex 3: to the end of the table; 4: none
    bad_faces = f.copy()
    bad_faces[3, 1] = 7
    for name, args in (("corners", (v5, f, offsets, bad_corners)),
                       ("offsets", (v5, f, bad_offsets, corners)),
                       ("faces", (v5, bad_faces, offsets, corners)),
                       ("all", (v5, bad_faces, bad_offsets, bad_corners))):
        want_bad = at.area_normals(*args)
        got = _normals(ctx, *args)
        assert np.isfinite(got).all(), name
        assert np.array_equal(got.view(np.int32), want_bad.view(np.int32)), name
    got = _normals(ctx, v5, f, offsets, bad_corners)
    assert np.array_equal(got[2:], want[2:]) and not np.array_equal(got[0], want[0])


# ----------------------------------------------------------------------------- d. refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    v, f = at.tetrahedron()
    offsets, corners = at.corner_table(f, 4)
    dv, df, do, dc = h.cuda(v), h.cuda(f), h.cuda(offsets), h.cuda(corners)
    out = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    good = [4, _ptr(dv), 4, _ptr(df), _ptr(do), _ptr(dc), _ptr(out)]
    for at_, value in [(0, -1), (2, -1), (1, null), (3, null), (4, null), (5, null), (6, null),
                       (0, (1 << 31) - 1), (2, 715827883)]:
        args = list(good)
        args[at_] = value
        assert ctx.lib.rn_vertex_area_normals(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_vertex_area_normals" in last(ctx._h)
    assert ctx.lib.rn_vertex_area_normals(ctx._h, 0, null, 0, null, null, null, null,
                                          _stream()) == _lib.RN_OK
    points, normals, cameras, images, depths = _scene(2, 24, 32, 3, seed=1)
    dp, dn, dcam, dimg, ddep = [h.cuda(a) for a in (points, normals, cameras, images, depths)]
    colors = torch.full((300, 3), -7.0, dtype=torch.float32, device="cuda")
    weight = torch.full((300,), -7.0, dtype=torch.float32, device="cuda")
    views = torch.full((300,), -7, dtype=torch.int32, device="cuda")
    #       0    1         2         3  4          5   6   7  8          9          10   11   12   13
    good = [300, _ptr(dp), _ptr(dn), 2, _ptr(dcam), 24, 32, 3, _ptr(dimg), _ptr(ddep), 0.1, 0.2, 1.5, 0,
            _ptr(colors), _ptr(weight), _ptr(views)]
    nan, inf = float("nan"), float("inf")
    for at_, value in [(0, -1), (1, null), (3, -1), (3, 33), (4, null), (5, 0), (6, 0), (5, -24),
                       (7, 0), (7, 5), (8, null), (10, -0.1), (10, nan), (10, inf), (11, -0.2),
                       (11, 1.0), (11, nan), (12, -1.5), (12, nan), (12, inf), (13, 2), (13, -1),
                       (14, null), (15, null), (16, null), (0, 715827883)]:
        args = list(good)
        args[at_] = value
        assert ctx.lib.rn_project_colors(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_project_colors" in last(ctx._h)
    torch.cuda.synchronize()
    assert (out == -7).all() and (colors == -7).all() and (weight == -7).all() and (views == -7).all()
    # what is NOT refused: no normals, no depths, no rows
    args = list(good)
    args[2] = args[9] = null
    assert ctx.lib.rn_project_colors(ctx._h, *args, _stream()) == _lib.RN_OK
    args = [0] + [null] * 2 + [2, null, 24, 32, 3, null, null, 0.1, 0.2, 1.5, 0, null, null, null]
    assert ctx.lib.rn_project_colors(ctx._h, *args, _stream()) == _lib.RN_OK
    # the wrappers raise with the entry's name
    with pytest.raises(_lib.RaynetHipError, match="rn_project_colors"):
        ctx.project_colors(dp, dn, dcam, dimg, ddep, -1.0, 0.0, 0.0, 0, colors, weight, views)
    from raynet_amd.appearance import project_colors
    cams, imgs, _ = at.plane_scene()
    with pytest.raises(ValueError, match="choose the\\s+frames"):
        project_colors(points, cams * 11, list(imgs) * 11)


# ------------------------------------------------------------------------------ e. the chain
def _write_scene(path, golden, cameras, images, depth_maps):
    """A Restrepo scene directory of the given cameras, images (written as 8-bit PNG) and
    ground-truth depth maps."""
    import shutil
    from PIL import Image as PILImage
    for d in ("imgs", "cams_krt", "gt"):
        os.makedirs(os.path.join(path, d))
    shutil.copy(os.path.join(golden, "restrepo_mock_scene_1", "scene_info.xml"),
                os.path.join(path, "scene_info.xml"))
    for i, (cam, image, depth) in enumerate(zip(cameras, images, depth_maps)):
        PILImage.fromarray(np.round(image * 255).astype(np.uint8)).save(
            os.path.join(path, "imgs", "frame_%03d.png" % i))
        with open(os.path.join(path, "cams_krt", "frame_%03d.txt" % i), "w") as f:
            for row in np.asarray(cam.K, D):
                f.write(" ".join("%.9g" % x for x in row) + "\n")
            f.write("\n")
            for row in np.asarray(cam.R, D):
                f.write(" ".join("%.9g" % x for x in row) + "\n")
            f.write("\n" + " ".join("%.9g" % x for x in np.asarray(cam.t, D).ravel()) + "\n")
        np.save(os.path.join(path, "gt", "gt_depth_%d.npy" % i), depth)


def test_from_a_forward_pass_to_a_coloured_mesh_and_coloured_clouds(tmp_path):
    from conftest import GOLDEN
    from raynet_amd.appearance import to_rgb8
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.common.mesh_io import parse_gt_data_from_ply, read_ply
    from raynet_amd.common.scene import Image, Scene, get_scene
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.scripts import convert_to_pointcloud, render_volume
    from raynet_amd.synthetic import make_synthetic_scene
    from raynet_amd.volume import SurfaceMesh
    H, W, grid = 20, 30, (18, 22, 14)
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=3, focal=1.5 * H)
    gp = GenerationParameters(depth_planes=16, neighbors=2, grid_shape=np.array(grid, np.int32),
                              max_number_of_marched_voxels=96, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    predicted = [np.array(m) for m in fp.forward_pass(scene, (0, 3, 1))]
    volume = fp.occupancy_volume()
    mesh = volume.mesh()
    assert not mesh.empty and mesh.normals is None and mesh.colors is None
    # synthetic images on the scene's cameras: a smooth, deterministic pattern per view
    yy, xx = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    images = [np.stack([0.5 + 0.5 * np.sin(0.3 * xx + k), 0.5 + 0.5 * np.cos(0.4 * yy - k),
                        (xx + 2 * yy + 7 * k) % 16 / 15.0], -1).astype(F) for k in range(3)]
    cameras = [scene.get_image(k).camera for k in range(3)]
    pictured = Scene([Image(im, cam) for im, cam in zip(images, cameras)], volume.bbox)
    bbox = volume.bbox.astype(D)
    tol = float(np.sqrt((((bbox[3:] - bbox[:3]) / np.array(grid)) ** 2).sum()))
    for mode in ("blend", "best"):
        views = mesh.colorize(pictured, [0, 1, 2], tol, min_cos=0.1, mode=mode)
        assert mesh.colors.dtype == np.uint8 and mesh.colors.shape == mesh.vertices.shape
        assert mesh.normals.dtype == F and views.dtype == np.uint32 and views.shape == (len(mesh.vertices),)
        # ... and they are the definition's, on the same depth maps and normals
        caster = mesh.raycaster()
        depth_maps = np.stack([caster.depth_map(cam, H, W).cpu().numpy() for cam in cameras])
        want = at.project_colors(mesh.vertices, mesh.normals, at.pack_cameras(cameras),
                                 np.stack(images), depth_maps, tol, 0.1, 0.0,
                                 0 if mode == "blend" else 1)
        assert np.array_equal(views, want[2])
        assert np.array_equal(mesh.colors, to_rgb8(want[0], want[2] != 0, (0.5, 0.5, 0.5)))
        assert (mesh.colors[views == 0] == 128).all()
    unit = at.area_normals(mesh.vertices, mesh.faces).astype(D)
    length = np.sqrt((unit ** 2).sum(1, keepdims=True))
    assert np.allclose(mesh.normals, unit / np.where(length > 0, length, 1), atol=1e-6)
    count = np.array([bin(m).count("1") for m in views])
    print("mesh: %d vertices; seen by 0 / 1 / 2 / 3 views: %s"
          % (len(mesh.vertices), np.bincount(count, minlength=4).tolist()))
    assert (count >= 2).any() and (count == 0).any()
    # the file: normals and colours come back
    path = str(tmp_path / "coloured.ply")
    mesh.save_ply(path)
    again = SurfaceMesh.load_ply(path)
    assert np.array_equal(again.vertices.view(np.int32), mesh.vertices.view(np.int32))
    assert np.array_equal(again.faces, mesh.faces) and np.array_equal(again.colors, mesh.colors)
    assert np.array_equal(again.normals.view(np.int32), mesh.normals.view(np.int32))
    points, rest, faces = parse_gt_data_from_ply(path)
    assert rest.shape == (len(points), 6) and np.array_equal(faces, mesh.faces)

    # render_volume --mesh --color on the scene as a directory (8-bit images, cameras as text)
    scene_dir, out = str(tmp_path / "scene"), str(tmp_path / "out")
    _write_scene(scene_dir, GOLDEN, cameras, images, [np.ones((H, W), F)] * 3)
    occupancy = str(tmp_path / "occupancy.npz")
    volume.save(occupancy)
    plain, coloured = str(tmp_path / "plain.ply"), str(tmp_path / "cli.ply")
    assert render_volume.main([scene_dir, occupancy, out, "--start_end", "0,0", "--mesh", plain]) == 0
    assert render_volume.main([scene_dir, occupancy, out, "--start_end", "0,3", "--mesh", coloured,
                               "--color", "--color_mode", "best"]) == 0
    bare = volume.mesh()
    bare.save_ply(str(tmp_path / "bare.ply"))
    assert open(plain, "rb").read() == open(str(tmp_path / "bare.ply"), "rb").read()
    cli = SurfaceMesh.load_ply(coloured)
    assert np.array_equal(cli.vertices.view(np.int32), mesh.vertices.view(np.int32))
    assert np.array_equal(cli.normals.view(np.int32), mesh.normals.view(np.int32))
    on_disk = get_scene("restrepo", scene_dir)
    cli_views = bare.colorize(on_disk, [0, 1, 2], tol, mode="best")
    assert np.array_equal(cli.colors, bare.colors)
    assert (cli_views != 0).any() and len(np.unique(cli.colors, axis=0)) > 10

    # convert_to_pointcloud --color on the pass's depth maps
    preds, clouds = str(tmp_path / "predictions"), str(tmp_path / "clouds")
    os.makedirs(preds)
    for i, m in enumerate(predicted):
        np.save(os.path.join(preds, "depth_%03d.npy" % i), m)
    convert_to_pointcloud.main([scene_dir, preds, clouds, "--borders", "2"])
    assert sorted(os.listdir(clouds)) == ["predicted_pc_s_0.ply"]
    before = open(os.path.join(clouds, "predicted_pc_s_0.ply"), "rb").read()
    convert_to_pointcloud.main([scene_dir, preds, clouds, "--borders", "2", "--color",
                                "--consistency_threshold", "0.1"])
    assert sorted(os.listdir(clouds)) == ["colored_predicted_pc_s_0.ply", "predicted_pc_s_0.ply"]
    assert open(os.path.join(clouds, "predicted_pc_s_0.ply"), "rb").read() == before
    vertex = read_ply(os.path.join(clouds, "colored_predicted_pc_s_0.ply"))["vertex"]
    xyz = np.stack([vertex[k] for k in "xyz"], 1)
    rgb = np.stack([vertex[k] for k in ("red", "green", "blue")], 1)
    assert len(xyz) == 3 * (H - 4) * (W - 4) and rgb.dtype == np.uint8
    # a point back-projected from a frame's own depth map is seen by that frame at least: its
    # colour is its pixel's, and nothing is left grey
    from raynet_amd.pointcloud import Pointcloud
    colors, cloud_views = Pointcloud(np.ascontiguousarray(xyz.T)).colorize(
        on_disk, [0, 1, 2], [os.path.join(preds, "depth_%03d.npy" % i) for i in range(3)], tol=0.1)
    assert np.array_equal(colors, rgb)
    per_frame = (H - 4) * (W - 4)
    for k in range(3):
        own = cloud_views[k * per_frame:(k + 1) * per_frame]
        assert ((own >> k) & 1).mean() > 0.99, k
    want = at.project_colors(
        xyz, None, at.pack_cameras([on_disk.get_image(k).camera for k in range(3)]),
        np.stack([on_disk.get_image(k).image for k in range(3)]), np.stack(predicted), 0.1, 0.0,
        0.0, 0)
    assert np.array_equal(cloud_views, want[2])
    assert np.array_equal(colors, to_rgb8(want[0], want[2] != 0))
