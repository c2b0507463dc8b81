"""Taubin smoothing on the GPU: rn_mesh_smooth against tests/smooth_truth.py
-- vertices_out EQUALS the truth's bits, vertices_in is what it was, the rows behind the output and
the bytes behind the workspace keep their prefill -- over the sizes at which a launch can go wrong:
nothing, one vertex, no faces, one triangle, a tetrahedron, strips around the wavefront and the
workgroup and one across many workgroups, stars whose hub has one long row, a closed and an open
iso-surface, both parities of the ping-pong, plain Laplacian steps, the clamp, non-finite
positions, garbage in all three index arrays, three launches that give one array, the entry's
refusals, and the chain from noisy depth maps of two spheres through the command line to a mesh
whose normals are better than the unsmoothed one's."""
import ctypes
import os
import re

import numpy as np
import pytest

import appearance_truth as at
import components_truth as ct
import isosurface_truth as it
import mesh_harness as h
import smooth_truth as st

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
FILL = -7.5
INF = float("inf")
NO_FACES = np.zeros((0, 3), np.int32)


def _launch(vertices, faces, offsets, corners, fixed, iterations, lam, mu, max_move):
    """rn_mesh_smooth on device tensors, the output PAD rows longer than nv and the workspace TAIL
    bytes longer than reported, both prefilled -> (rc, out with its pad, the four inputs
    afterwards, the workspace, the bytes it needs)."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    nv, nf = len(vertices), len(faces)
    v, f = h.cuda(np.reshape(vertices, (-1, 3)), F), h.cuda(np.reshape(faces, (-1, 3)), np.int32)
    o, c, fx = h.cuda(offsets, np.int32), h.cuda(corners, np.int32), h.cuda(fixed, np.uint8)
    need = int(ctx.lib.rn_mesh_smooth_workspace_bytes(ctx._h, nv, nf))
    assert need == (24 * nf + 12 * nv + 7) // 8 * 8
    work, out = h.workspace(need), h.padded((nv, 3), FILL, torch.float32)
    rc = ctx.lib.rn_mesh_smooth(ctx._h, nv, _ptr(v), nf, _ptr(f), _ptr(o), _ptr(c), _ptr(fx),
                                int(iterations), float(lam), float(mu), float(max_move),
                                _ptr(work), _ptr(out), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), (v, f, o, c), work, need


def _same_as_truth(vertices, faces, what, iterations=10, lam=0.5, mu=-0.53, fixed=None,
                   max_move=INF, offsets=None, corners=None, nan_payloads=False):
    """vertices_out has the truth's bits, the inputs their own, the pads their prefill -> out."""
    from raynet_amd import _lib
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    nv = len(vertices)
    if offsets is None:
        offsets, corners = at.corner_table(faces, nv)
    want = st.smooth(vertices, faces, iterations, lam, mu, fixed, max_move, offsets, corners)
    rc, out, after, work, need = _launch(vertices, faces, offsets, corners, fixed, iterations, lam,
                                         mu, max_move)
    assert rc == _lib.RN_OK, what
    h.assert_untouched(out, nv, FILL, (what, "vertices_out"))
    h.assert_untouched(work, need, h.TAIL_BYTE, (what, "the workspace"))
    for tensor, uploaded in zip(after, (vertices, np.reshape(faces, (-1, 3)), offsets, corners)):
        h.assert_input_kept(tensor, uploaded, what)
    h.assert_same_bits(out[:nv], want, what, nan_payloads)
    return out[:nv]


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
    assert not st.boundary_vertices(faces, len(vertices)).any()
    return vertices, faces


# ------------------------------------------------------------------------------ a. sizes
@pytest.mark.parametrize("faces,nv", [(NO_FACES, 0), (NO_FACES, 1), (NO_FACES, 5),
                                      (np.array([[0, 1, 2]], np.int32), 3),
                                      (ct.tetrahedra(1)[0], 4)],
                         ids=["nv 0", "nv 1", "nv 5, no faces", "one triangle", "one tetrahedron"])
def test_empty_and_trivial(faces, nv):
    vertices = st.positions(nv, seed=nv)
    out = _same_as_truth(vertices, faces, "trivial")
    if len(faces) == 0:
        assert np.array_equal(h.bits(out), h.bits(vertices))
    else:
        assert (h.bits(out) != h.bits(vertices)).any(1).all()
        _same_as_truth(vertices, faces, "trivial, 1 iteration", iterations=1)
        _same_as_truth(vertices, faces, "trivial, no iteration", iterations=0)


@pytest.mark.parametrize("permuted", [False, True], ids=["ascending", "permuted"])
@pytest.mark.parametrize("nv", [3, 64, 65, 256, 257, 20003])
def test_strips(nv, permuted):
    vertices, faces = st.strip(nv, seed=nv, permuted=permuted)
    _same_as_truth(vertices, faces, "strip %d" % nv)


@pytest.mark.parametrize("hub_last", [False, True], ids=["vertex 0", "the last vertex"])
def test_one_long_row_among_short_ones(hub_last):
    vertices, faces = st.star(500, seed=5, hub_last=hub_last)
    out = _same_as_truth(vertices, faces, "star")
    hub = len(vertices) - 1 if hub_last else 0
    assert (h.bits(out[hub]) != h.bits(vertices[hub])).any()


# ------------------------------------------------------------------------------ b. iso-surfaces
def test_the_closed_iso_surface_of_the_binary_ball(ball):
    vertices, faces = ball
    out = _same_as_truth(vertices, faces, "ball")
    # what the smoothing is for, on the GPU's own result
    assert st.mean_angle_to_radial(out, faces, st.BALL_CENTRE) < \
        st.mean_angle_to_radial(vertices, faces, st.BALL_CENTRE)


def test_the_open_iso_surface_of_the_cut_ball_with_its_border_pinned():
    import torch
    from raynet_amd.fusion import _grid_context
    from raynet_amd.smoothing import boundary_vertices, smooth_vertices
    field = it.cut_ball()
    bbox, _ = it.unit_frame(field.shape)
    ctx = _grid_context(bbox, field.shape)
    vertices, faces = ctx.isosurface(torch.from_numpy(field).cuda(), 0.5, False)
    border = boundary_vertices(faces, len(vertices)).cpu().numpy()
    vertices, faces = vertices.cpu().numpy(), faces.cpu().numpy()
    want_border = st.boundary_vertices(faces, len(vertices))
    assert 0 < want_border.sum() < len(vertices) and np.array_equal(border, want_border)
    out = _same_as_truth(vertices, faces, "cut ball", fixed=want_border)
    assert np.array_equal(h.bits(out[want_border]), h.bits(vertices[want_border]))
    # the wrapper pins the same vertices by itself
    assert np.array_equal(h.bits(smooth_vertices(vertices, faces, fixed="boundary")), h.bits(out))
    free = smooth_vertices(vertices, faces, fixed=None)
    assert np.array_equal(h.bits(free), h.bits(st.smooth(vertices, faces)))
    assert (h.bits(free[want_border]) != h.bits(vertices[want_border])).any()


# ------------------------------------------------------------------ c. step counts and parameters
@pytest.mark.parametrize("kw", [dict(iterations=1), dict(iterations=2), dict(iterations=3),
                                dict(iterations=10), dict(iterations=1, mu=0.0),
                                dict(iterations=2, mu=0.0), dict(max_move=0.05),
                                dict(max_move=None)],
                         ids=lambda kw: " ".join("%s=%s" % i for i in kw.items()))
def test_step_counts_and_parameters_on_the_ball(ball, kw):
    vertices, faces = ball
    kw = dict(kw)
    if "max_move" in kw and kw["max_move"] is None:
        kw["max_move"] = INF
    out = _same_as_truth(vertices, faces, str(kw), **kw)
    if kw.get("max_move", INF) < INF:
        lo, hi = st.clamp_bounds(vertices, kw["max_move"])
        assert (out >= lo).all() and (out <= hi).all() and ((out == lo) | (out == hi)).any()


def test_non_finite_positions_spread_to_their_neighbours_only(ball):
    vertices, faces = ball
    v = vertices.copy()
    v[17, 1], v[1500, 2] = np.nan, np.inf
    out = _same_as_truth(v, faces, "one NaN, one inf, one step", iterations=1, mu=0.0,
                         nan_payloads=True)
    near = np.zeros(len(v), bool)
    near[faces[((faces == 17) | (faces == 1500)).any(1)].reshape(-1)] = True
    assert np.array_equal(~np.isfinite(out).all(1), near)
    _same_as_truth(v, faces, "one NaN, one inf", iterations=3, max_move=0.25, nan_payloads=True)


def test_garbage_in_all_three_index_arrays_reads_nothing_out_of_bounds(ball):
    vertices, faces = ball
    nv, nf = len(vertices), len(faces)
    offsets, corners = at.corner_table(faces, nv)
    bad_faces, hit = st.with_bad_faces(faces, nv, seed=21)
    assert 0.02 * nf < hit.sum() < 0.1 * nf
    _same_as_truth(vertices, bad_faces, "bad faces", iterations=2, offsets=offsets, corners=corners)
    bad_corners, hit = st.with_bad_corners(corners, nf, seed=22)
    assert 0.02 * 3 * nf < hit.sum() < 0.1 * 3 * nf
    _same_as_truth(vertices, faces, "bad corners", iterations=2, offsets=offsets,
                   corners=bad_corners)
    # reversed, negative and overhanging ranges as well, everything at once, on a small mesh too
    bad_offsets = offsets.copy()
    rng = np.random.default_rng(23)
    where = rng.choice(nv + 1, 150, replace=False)
    bad_offsets[where] = rng.choice(np.array([-1, -2 ** 31, 3 * nf + 1, 2 ** 31 - 1, 0, 3 * nf],
                                             np.int64), 150).astype(np.int32)
    out = _same_as_truth(vertices, bad_faces, "bad everything", iterations=2, offsets=bad_offsets,
                         corners=bad_corners)
    assert np.isfinite(out).all()
    v, f = st.strip(65, seed=24, permuted=True)
    o, c = at.corner_table(f, 65)
    o[[3, 30, 64]] = [-5, 10 ** 6, -2 ** 31]
    _same_as_truth(v, st.with_bad_faces(f, 65, 25, 0.2)[0], "bad strip", offsets=o,
                   corners=st.with_bad_corners(c, len(f), 26, 0.2)[0])
    # nothing but garbage: nothing moves
    only = np.array([[-1, 0, 1], [0, 5, 1], [2 ** 31 - 1, 0, 1], [0, 1, -2 ** 31]], np.int64)
    p = st.positions(5, 27)
    out = _same_as_truth(p, only.astype(np.int32), "only garbage", offsets=[0, 4, 8, 8, 8, 8],
                         corners=[0, 3, 4, 7, 9, 10, 2, 5, 1, 6, 8, 11])
    assert np.array_equal(h.bits(out), h.bits(p))


def test_three_launches_give_one_array():
    from raynet_amd import _lib
    vertices, faces = st.strip(20003, seed=20003, permuted=True)
    offsets, corners = at.corner_table(faces, 20003)
    runs = [_launch(vertices, faces, offsets, corners, None, 10, 0.5, -0.53, INF) for _ in range(3)]
    for run in runs:
        assert run[0] == _lib.RN_OK
        assert np.array_equal(h.bits(run[1]), h.bits(runs[0][1]))


# ------------------------------------------------------------------------------ d. refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    from raynet_amd.smoothing import smooth_vertices
    ctx = h.ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    vertices_np, faces_np = st.strip(40, seed=1, permuted=True)
    nv, nf = 40, len(faces_np)
    offsets_np, corners_np = at.corner_table(faces_np, nv)
    v, f = torch.from_numpy(vertices_np).cuda(), torch.from_numpy(faces_np).cuda()
    o, c = torch.from_numpy(offsets_np).cuda(), torch.from_numpy(corners_np).cuda()
    need = int(ctx.lib.rn_mesh_smooth_workspace_bytes(ctx._h, nv, nf))
    work = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((nv, 3), FILL, dtype=torch.float32, device="cuda")

    def at_(p, byte):
        return ctypes.c_void_p(p.value + byte)

    #       0   1        2   3        4        5        6     7   8    9      10   11          12
    good = [nv, _ptr(v), nf, _ptr(f), _ptr(o), _ptr(c), null, 10, 0.5, -0.53, INF, _ptr(work), _ptr(out)]
    nan = float("nan")
    for where, value in [(0, -1), (2, -1), (0, 2 ** 31 - 1), (0, 2 ** 40), (2, (2 ** 31 - 1) // 3 + 1),
                      (2, 2 ** 40), (7, -1), (7, 10001), (8, 0.0), (8, -0.5), (8, 1.5), (8, nan),
                      (8, INF), (9, 0.25), (9, -1.5), (9, nan), (9, -INF), (10, 0.0), (10, -1.0),
                      (10, nan), (1, null), (4, null), (12, null), (11, null), (3, null), (5, null),
                      (11, at_(_ptr(work), 4)), (11, at_(_ptr(work), 1)), (12, _ptr(v)),
                      (12, _ptr(work)), (1, _ptr(work))]:
        args = list(good)
        args[where] = value
        assert ctx.lib.rn_mesh_smooth(ctx._h, *args, _stream()) == INVALID, (where, value)
        assert b"rn_mesh_smooth" in last(ctx._h), (where, value)
    assert ctx.lib.rn_mesh_smooth_workspace_bytes(ctx._h, -1, 0) == -1
    assert b"rn_mesh_smooth_workspace_bytes" in last(ctx._h)
    assert ctx.lib.rn_mesh_smooth_workspace_bytes(ctx._h, 0, 2 ** 40) == -1
    assert ctx.lib.rn_mesh_smooth_workspace_bytes(ctx._h, 2 ** 31 - 1, 0) == -1
    torch.cuda.synchronize()
    assert (out == FILL).all() and (work == 0xA5).all()
    assert np.array_equal(h.bits(v.cpu().numpy()), h.bits(vertices_np))
    # what is NOT refused: no faces and no pointers to them; nothing at all; the limits
    assert ctx.lib.rn_mesh_smooth(ctx._h, nv, _ptr(v), 0, null, _ptr(o), null, *good[6:],
                                  _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert np.array_equal(h.bits(out.cpu().numpy()), h.bits(vertices_np))
    assert ctx.lib.rn_mesh_smooth(ctx._h, 0, null, 0, null, null, null, null, 10, 0.5, -0.53, INF,
                                  null, null, _stream()) == _lib.RN_OK
    for where, value in [(7, 0), (8, 1.0), (9, -1.0), (9, 0.0), (10, 1e-300),
                      (11, at_(_ptr(work), 8))]:
        args = list(good)
        args[where] = value
        assert ctx.lib.rn_mesh_smooth(ctx._h, *args, _stream()) == _lib.RN_OK, (where, value)
    torch.cuda.synchronize()
    # the context method: what it returns, and tensors that are not what the kernels read
    got = ctx.mesh_smooth(v, f, o, c)
    assert got.dtype == torch.float32 and tuple(got.shape) == (nv, 3)
    assert np.array_equal(h.bits(got.cpu().numpy()), h.bits(st.smooth(vertices_np, faces_np)))
    pins = torch.zeros((nv,), dtype=torch.uint8, device="cuda")
    pins[::4] = 1
    given = ctx.mesh_smooth(v, f, o, c, fixed=pins, iterations=3, lam=0.4, mu=-0.45, max_move=0.5,
                            workspace=work, out=out)
    assert given is out and np.array_equal(
        h.bits(out.cpu().numpy()),
        h.bits(st.smooth(vertices_np, faces_np, 3, 0.4, -0.45, pins.cpu().numpy(), 0.5)))
    for bad, match in [
            (dict(vertices=v.double()), "vertices"), (dict(vertices=v.cpu()), "vertices"),
            (dict(faces=f.long()), "faces"), (dict(offsets=o[:-1]), "offsets"),
            (dict(offsets=o.long()), "offsets"), (dict(corners=c[:-1]), "corners"),
            (dict(fixed=pins.bool()), "fixed"), (dict(fixed=pins[:-1]), "fixed"),
            (dict(workspace=work[:need - 8]), "workspace"), (dict(workspace=work[4:]), "workspace"),
            (dict(out=out[:-1]), "out"), (dict(out=out.double()), "out")]:
        kw = dict(vertices=v, faces=f, offsets=o, corners=c)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            ctx.mesh_smooth(**kw)
    with pytest.raises(_lib.RaynetHipError, match="rn_mesh_smooth"):
        ctx.mesh_smooth(v, f, o, c, out=v)
    # the wrapper raises its ValueErrors with a GPU as without one
    for kw, match in [(dict(iterations=-1), "iterations"), (dict(lam=0.0), "lam"),
                      (dict(mu=0.5), "mu"), (dict(max_move=0.0), "max_move"),
                      (dict(fixed=np.zeros(3, bool)), "fixed")]:
        with pytest.raises(ValueError, match=match):
            smooth_vertices(vertices_np, faces_np, **kw)


# ------------------------------------------------------------------------------ e. the chain
def test_from_noisy_maps_of_two_spheres_to_a_smoother_mesh(tmp_path, capsys):
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
    rough_ply, smooth_ply = str(tmp_path / "rough.ply"), str(tmp_path / "smooth.ply")
    cloud_ply = str(tmp_path / "smooth_cloud.ply")
    assert fuse_depth_maps.main([scene_dir, preds, rough_ply] + common) == 0
    assert "smooth:" not in capsys.readouterr().out
    assert fuse_depth_maps.main([scene_dir, preds, smooth_ply, "--smooth", "5", "--mesh_cloud",
                                 cloud_ply, "--mesh_samples", "2000", "--seed", "3"] + common) == 0
    printed = capsys.readouterr().out
    rough, smooth = SurfaceMesh.load_ply(rough_ply), SurfaceMesh.load_ply(smooth_ply)
    assert np.array_equal(smooth.faces, rough.faces) and len(smooth.vertices) == len(rough.vertices)
    # the vertices are the truth's, from the unsmoothed file's: the border pinned, one side of
    # the smallest voxel the limit
    side = float((2.0 / np.array(grid, D)).min())
    border = st.boundary_vertices(rough.faces, len(rough.vertices))
    want = st.smooth(rough.vertices, rough.faces, 5, 0.5, -0.53, border, side)
    assert np.array_equal(h.bits(smooth.vertices), h.bits(want))
    # the printed line, and the farthest move within the default limit
    m = re.search(r"^smooth: 5 iterations, (\d+) vertices, farthest move ([0-9.]+) voxel sides$",
                  printed, re.M)
    assert m is not None, printed
    far = float(np.abs(smooth.vertices.astype(D) - rough.vertices.astype(D)).max()) / side
    assert int(m.group(1)) == len(rough.vertices) and m.group(2) == "%.3f" % far
    assert 0.0 < far <= 1.0
    # the normals of the file are the smoothed surface's, and they are better: the unsmoothed
    # run is the yardstick
    assert smooth.normals is not None and rough.normals is not None
    before = st.mean_angle_to_radial(rough.vertices, rough.faces, big[0], rough.normals)
    after = st.mean_angle_to_radial(smooth.vertices, smooth.faces, big[0], smooth.normals)
    print("mean angle to the large sphere's radial direction: %.2f deg unsmoothed, %.2f deg "
          "smoothed; farthest move %.3f voxel sides" % (before, after, far))
    assert after < before
    # the cloud is sampled from the smoothed mesh and goes into the accuracy metric (1e-5 of the
    # box's largest coordinate: the bound tests/test_components_gpu.py uses for the same statement)
    cli_points = parse_stl_file_to_pointcloud(cloud_ply)
    assert cli_points.shape == (2000, 3)
    dist, _, _ = smooth.raycaster().closest_points(cli_points)
    assert float(dist.max()) <= 1e-5
    args = compute_metrics.build_parser().parse_args(
        [scene_dir, str(tmp_path), "accuracy", "--use_pc_from_depthmap", "--borders", "4"])
    values, _ = compute_metrics.build_metric("accuracy", args).compute(
        on_disk, [0, 1], None, Pointcloud(np.ascontiguousarray(cli_points.T)))
    assert np.asarray(values).size == 2000 and np.isfinite(values).all()
