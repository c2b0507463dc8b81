"""The occupancy volume on the GPU: rn_occupancy_grid against the float64 definition,
rn_volume_render against tests/volume_truth.py bit for bit (the lists of the truth are the
library's own rn_voxel_traversal on the same segments), and both through a forward pass, a
file and a camera."""
import ctypes

import numpy as np
import pytest

import volume_truth as vt

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


def _context(M, grid=vt.GRID, bbox=vt.BBOX):
    from raynet_amd.common.scene import get_voxel_grid
    from raynet_amd.hip_implementations.context import HipContext
    ctx = HipContext(M, 2, 2, 1, 1, 1, 0, bbox, grid)
    vg = np.ascontiguousarray(get_voxel_grid(np.array(bbox, F), grid).transpose(1, 2, 3, 0))
    ctx.set_voxel_grid(vg)
    return ctx, vg


# ------------------------------------------------------------------------------- a. belief
@pytest.mark.parametrize("bias", [0.0, -2.94])
@pytest.mark.parametrize("grid", [(5, 6, 7), (8, 8, 8)])
def test_belief_grid(grid, bias):
    """Both accumulator layouts give the same bits, within 1e-6 of the float64 logistic of the
    fp32 sum (occupancy_to_ray's fast exponential: < 4e-7 on a value in (0, 1)), and the clamp
    constants exactly where the logistic lies beyond them."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx, _ = _context(8, grid, (0, 0, 0, 1, 1, 1))
    rng = np.random.default_rng(11)
    acc = rng.normal(0.0, 6.0, grid).astype(F)
    planted = np.repeat(np.array([9.2, -9.2, 9.3, -9.3, 40.0, -40.0], F), 16)
    where = rng.choice(acc.size, planted.size, replace=False)
    acc.reshape(-1)[where] = planted
    acc_grid = torch.from_numpy(acc).cuda()
    # the bricked buffer of the same values; NaN in the padding of the partial bricks
    acc_bricks = torch.full((ctx.acc_size(),), float("nan"), dtype=torch.float32, device="cuda")
    ctx._check(ctx.lib.rn_acc_from_grid(ctx._h, _ptr(acc_grid), _ptr(acc_bricks), _stream()))
    assert bool(torch.isnan(acc_bricks).any()) == any(g % 4 for g in grid)
    from_grid = ctx.occupancy_grid(acc_grid, False, bias).cpu().numpy()
    from_bricks = ctx.occupancy_grid(acc_bricks, True, bias).cpu().numpy()
    assert from_grid.shape == tuple(grid) and from_grid.dtype == F
    assert np.array_equal(_bits(from_grid), _bits(from_bricks))
    mu = (F(bias) + acc).astype(F)
    want = vt.belief64(mu)
    err = np.abs(from_grid.astype(np.float64) - want).max()
    print("belief grid %s bias %g: max |belief - belief64| = %.3g" % (grid, bias, err))
    assert err <= 1e-6
    raw = vt.sigmoid64(mu)
    high, low = raw > vt.HI + 1e-6, raw < vt.LO - 1e-6
    assert high.sum() >= 16 and low.sum() >= 16
    assert (from_grid[high] == F(1 - 1e-4)).all() and (from_grid[low] == F(1e-4)).all()
    inside = (raw > vt.LO + 1e-6) & (raw < vt.HI - 1e-6)
    assert inside.sum() >= 16 and (from_grid[inside] > F(1e-4)).all() and \
        (from_grid[inside] < F(1 - 1e-4)).all()


# ------------------------------------------------------------------------------- b. render
@pytest.fixture(scope="module")
def segments():
    import torch
    s, e = vt.make_segments()
    return s, e, torch.from_numpy(s).cuda(), torch.from_numpy(e).cuda()


def _traverse(ctx, starts, ends):
    import torch
    n = len(starts)
    rvi = torch.zeros((n, ctx.M, 3), dtype=torch.int32, device="cuda")
    rvc = torch.zeros((n,), dtype=torch.int32, device="cuda")
    ctx.voxel_traversal(starts, ends, rvi, rvc)
    return rvi.cpu().numpy(), rvc.cpu().numpy()


def _beliefs():
    rng = np.random.default_rng(23)
    plain = rng.uniform(1e-4, 1 - 1e-4, vt.GRID).astype(F)
    wall = plain.copy()
    wall[9] = F(1 - 1e-4)
    return {"random": plain, "random + wall at x = 9": wall}


@pytest.mark.parametrize("M", [40, 7])
def test_render_is_the_restatement_bit_for_bit(M, segments):
    import torch
    ctx, vg = _context(M)
    s, e, starts, ends = segments
    n = len(s)
    assert n == 197 and n % 64
    rvi, rvc = _traverse(ctx, starts, ends)
    # the fixture, from the library's own lists
    assert (rvc == 0).sum() >= 30
    if M == 7:
        assert (rvc == 7).sum() >= 60 and rvc.max() == 7
    else:
        assert rvc.max() < M and rvc[rvc > 0].min() <= 1 and rvc.max() >= 20
    center = torch.tensor(vt.CENTER, dtype=torch.float32, device="cuda")
    for name, belief in _beliefs().items():
        out = torch.full((5, n + 5), -7.0, dtype=torch.float32, device="cuda")
        ctx.volume_render(starts, ends, center, torch.from_numpy(belief).cuda(), out)
        got = out.cpu().numpy()
        assert (got[:, n:] == -7).all(), "written beyond n"
        want = vt.render32(rvi, rvc, belief, vg, vt.CENTER)
        assert np.isfinite(got[:, :n]).all()
        for k, plane in enumerate(vt.PLANES):
            diff = np.abs(got[k, :n].astype(np.float64) - want[k]).max()
            print("M %d %s %s: max |diff| = %.3g" % (M, name, plane, diff))
            assert np.array_equal(_bits(got[k, :n]), _bits(want[k])), (name, plane, diff)
        assert not got[:, :n][:, rvc == 0].any()


# --------------------------------------------------------------------------- c. front wall
def test_front_wall(segments):
    import torch
    ctx, vg = _context(40)
    s, e, starts, ends = segments
    n = len(s)
    rvi, rvc = _traverse(ctx, starts, ends)
    belief = torch.full(vt.GRID, float(F(1 - 1e-4)), dtype=torch.float32, device="cuda")
    center = torch.tensor(vt.CENTER, dtype=torch.float32, device="cuda")
    out = torch.empty((5, n), dtype=torch.float32, device="cuda")
    ctx.volume_render(starts, ends, center, belief, out)
    depth, opacity, _, confidence, median = out.cpu().numpy()
    hit = rvc > 0
    assert hit.sum() >= 150
    first = vt.voxel_distance32(rvi[hit, 0], vg, vt.CENTER)
    assert np.array_equal(depth[hit], first) and np.array_equal(median[hit], depth[hit])
    assert (opacity[hit] >= F(1 - 1e-4)).all() and (confidence[hit] == F(1 - 1e-4)).all()
    assert not out.cpu().numpy()[:, ~hit].any()


# ------------------------------------------------------------ d. through the forward pass
def test_volume_of_a_forward_pass(tmp_path):
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.synthetic import make_synthetic_scene
    from raynet_amd.volume import OccupancyVolume, VolumeRender
    H, W, grid = 20, 30, (18, 22, 14)        # every axis ends in a partial brick
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=3, focal=1.5 * H)
    gp = GenerationParameters(depth_planes=16, neighbors=2, grid_shape=np.array(grid, np.int32),
                              max_number_of_marched_voxels=96, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    with pytest.raises(RuntimeError, match="needs a finished forward pass"):
        fp.occupancy_volume()
    maps = list(fp.forward_pass(scene, (0, 3, 1)))
    assert len(maps) == 3 and fp.schedule == "resident"
    volume = fp.occupancy_volume()
    assert isinstance(volume, OccupancyVolume) and volume.grid_shape == grid
    assert np.array_equal(volume.bbox, scene.bbox.ravel().astype(F))
    belief = volume.belief.cpu().numpy()
    want = vt.belief64(fp.accumulator.cpu().numpy())
    err = np.abs(belief.astype(np.float64) - want).max()
    print("forward pass: max |belief - belief64(accumulator)| = %.3g" % err)
    assert belief.shape == grid and err <= 1e-6
    assert belief.min() >= F(1e-4) and belief.max() <= F(1 - 1e-4) and belief.std() > 0
    # save, load, render view 0: the live volume's render, bit for bit
    path = str(tmp_path / "occupancy.npz")
    volume.save(path)
    camera = scene.get_image(0).camera
    live = volume.render(camera, (H, W))
    loaded = OccupancyVolume.load(path).render(camera, (H, W))
    assert isinstance(live, VolumeRender)
    for name in VolumeRender.FIELDS:
        a, b = getattr(live, name), getattr(loaded, name)
        assert a.shape == (H, W) and a.dtype == F
        assert np.array_equal(_bits(a), _bits(b)), name
    assert np.isfinite(live.depth).all()
    assert (live.opacity >= 0).all() and (live.opacity <= 1).all() and live.opacity.max() > 0
    # render_scene is render per frame, and the maps are in the depth maps' orientation: view
    # 0's render of the volume and its depth map from the pass see the box in the same pixels
    again = list(volume.render_scene(scene, [0, 2]))
    assert len(again) == 2 and np.array_equal(_bits(again[0].depth), _bits(live.depth))
    assert ((live.depth != 0) == (maps[0] != 0)).mean() >= 0.95


def test_reference_schedule_gives_the_same_kind_of_volume():
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.synthetic import make_synthetic_scene
    H, W, grid = 8, 12, (10, 9, 6)
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=3, focal=1.5 * H)
    gp = GenerationParameters(depth_planes=8, neighbors=2, grid_shape=np.array(grid, np.int32),
                              max_number_of_marched_voxels=32, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0,
                                            schedule="reference")
    list(fp.forward_pass(scene, (0, 3, 1)))
    belief = fp.occupancy_volume().belief.cpu().numpy()
    want = vt.belief64(fp.accumulator.cpu().numpy())
    assert belief.shape == grid and np.abs(belief.astype(np.float64) - want).max() <= 1e-6


# --------------------------------------------------------------------- the entries' checks
def test_bad_arguments_are_refused_before_any_launch(segments):
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx, _ = _context(40)
    s, e, starts, ends = segments
    n = len(s)
    center = torch.tensor(vt.CENTER, dtype=torch.float32, device="cuda")
    belief = torch.full(vt.GRID, 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((5, n), -7.0, dtype=torch.float32, device="cuda")
    args = [_ptr(starts), _ptr(ends), _ptr(center), _ptr(belief), _ptr(out)]
    render = ctx.lib.rn_volume_render
    assert render(ctx._h, n, *args, n - 1, _stream()) == -1           # RN_ERR_INVALID
    assert b"rn_volume_render" in ctx.lib.rn_last_error(ctx._h)
    assert render(ctx._h, -1, *args, n, _stream()) == -1
    for k in range(5):
        bad = list(args)
        bad[k] = ctypes.c_void_p(0)
        assert render(ctx._h, n, *bad, n, _stream()) == -1
    assert render(ctx._h, 0, *[ctypes.c_void_p(0)] * 5, 0, _stream()) == _lib.RN_OK
    grid = ctx.lib.rn_occupancy_grid
    assert grid(ctx._h, ctypes.c_void_p(0), 0, 0.0, _ptr(belief), _stream()) == -1
    assert grid(ctx._h, _ptr(belief), 2, 0.0, _ptr(belief), _stream()) == -1
    torch.cuda.synchronize()
    assert (out == -7).all()
    with pytest.raises(ValueError):
        ctx.volume_render(starts, ends, center, belief, out[:, :n - 1].contiguous())
    # a context without a voxel grid cannot say how far a voxel is
    from raynet_amd.hip_implementations.context import HipContext
    bare = HipContext(40, 2, 2, 1, 1, 1, 0, vt.BBOX, vt.GRID)
    with pytest.raises(_lib.RaynetHipError, match="rn_set_voxel_grid"):
        bare.volume_render(starts, ends, center, belief, out)


# ------------------------------------------------------------------- the command lines
def test_command_lines_score_the_volume(tmp_path):
    """forward_pass --save_occupancy, render_volume, compute_metrics ppmde on a Restrepo directory
    of the mock cameras: the volume is scored by the tool that scores depth maps -- also from a
    frame the pass never took as a reference image."""
    import os

    from conftest import GOLDEN
    from raynet_amd.scripts import compute_metrics, forward_pass, render_volume
    from training_tree import write_plane_scene
    H, W, views = 45, 80, 5
    scene_dir, out, out2 = (str(tmp_path / d) for d in ("scene", "out", "out2"))
    write_plane_scene(scene_dir, GOLDEN, H=H, W=W, views=views)
    assert forward_pass.main([scene_dir, out, "--depth_planes", "16", "--grid_shape", "32,32,16",
                              "--maximum_number_of_marched_voxels", "96", "--start_end", "0,3",
                              "--save_occupancy"]) == 0
    assert sorted(os.listdir(out)) == ["depth_000.npy", "depth_001.npy", "depth_002.npy",
                                       "occupancy.npz"]
    ply = str(tmp_path / "voxels.ply")
    assert render_volume.main([scene_dir, os.path.join(out, "occupancy.npz"), out2,
                               "--start_end", "0,4", "--plane", "expected_depth",
                               "--ply", ply, "--threshold", "0.05", "--all_voxels"]) == 0
    assert sorted(os.listdir(out2)) == sorted(
        ["%s_%03d.npy" % (name, i) for name in ("depth", "opacity") for i in range(4)])
    for i in range(4):        # frame 3 was no reference image of the pass
        d = np.load(os.path.join(out2, "depth_%03d.npy" % i))
        o = np.load(os.path.join(out2, "opacity_%03d.npy" % i))
        assert d.shape == o.shape == (H, W) and d.dtype == o.dtype == F
        assert np.isfinite(d).all() and (o >= 0).all() and (o <= 1).all() and (d >= 0).all()
    with open(ply, "rb") as f:
        assert f.read(3) == b"ply"
    res = compute_metrics.main([scene_dir, out2, "ppmde", "--frame_idxs", "0:4", "--borders", "4",
                                "--output_directory", str(tmp_path / "pc")])
    assert set(res) == {"ppmde"} and len(res["ppmde"]) > 0 and np.isfinite(res["ppmde"]).all()
