"""The cross-view check on the command lines: without the new flags
fuse_depth_maps and convert_to_pointcloud parse as they did, the flags' errors, and -- on the GPU --
filter_depth_maps on the cameras and the box of tests/golden/restrepo_mock_scene_1 with synthetic
maps of the ground plane writes its three files per frame with the truth's counts, which
fuse_depth_maps and convert_to_pointcloud then take."""
import os

import numpy as np
import pytest

import consistency_truth as ct
import eval_truth as et
from conftest import REPO

F = np.float32
D = np.float64
MOCK = os.path.join(REPO, "tests", "golden", "restrepo_mock_scene_1")
NEW = ("min_consistent_views", "max_violations", "consistency_abs", "consistency_rel")


def test_without_the_new_flags_the_scripts_parse_as_before():
    from raynet_amd.scripts import convert_to_pointcloud, fuse_depth_maps
    a = fuse_depth_maps.build_parser().parse_args(["scene", "predictions", "out.ply"])
    assert all(getattr(a, name) is None for name in NEW)
    assert (a.truncation, a.min_weight, a.border, a.pred_suffix) == (None, 0.0, 0.0, "depth")
    assert not (a.gt or a.confidence_weights or a.normals or a.color) and a.volume is None
    b = convert_to_pointcloud.build_parser().parse_args(["scene", "predictions", "out"])
    assert all(getattr(b, name) is None for name in NEW)
    assert (b.borders, b.consistency_threshold, b.n_neighbors) == (40, 0.75, 5)
    assert not b.with_consistency_check and b.min_confidence is None and not b.color
    # given, they are what was typed; the defaults are filled in by the check
    from raynet_amd.scripts import consistency_flags
    a = fuse_depth_maps.build_parser().parse_args(
        ["s", "p", "o.ply", "--min_consistent_views", "3", "--consistency_abs", "0.05"])
    assert (a.min_consistent_views, a.max_violations, a.consistency_abs, a.consistency_rel) == \
        (3, None, 0.05, None)
    consistency_flags.check(fuse_depth_maps.build_parser(), a)
    assert (a.max_violations, a.consistency_abs, a.consistency_rel) == (0, 0.05, 0.01)
    assert consistency_flags.requested(a) and not consistency_flags.requested(b)


def test_the_flags_errors(tmp_path, capsys):
    from raynet_amd.scripts import convert_to_pointcloud, filter_depth_maps, fuse_depth_maps
    out = str(tmp_path / "out.ply")
    K = ["--min_consistent_views", "2"]
    for script, head, cases in [
            (fuse_depth_maps, ["scene", "predictions", out], [
                (["--max_violations", "1"], "--max_violations goes with"),
                (["--consistency_abs", "0.1"], "--consistency_abs goes with"),
                (["--consistency_rel", "0.1"], "--consistency_rel goes with"),
                (K + ["--gt"], "ground-truth depth maps are not checked"),
                (["--min_consistent_views", "-1"], "--min_consistent_views takes"),
                (K + ["--max_violations", "-1"], "--max_violations takes"),
                (K + ["--consistency_abs", "-0.1"], "--consistency_abs takes"),
                (K + ["--consistency_rel", "nan"], "--consistency_rel takes"),
                (K + ["--consistency_rel", "inf"], "--consistency_rel takes")]),
            (convert_to_pointcloud, ["scene", "predictions", str(tmp_path / "cloud")], [
                (["--max_violations", "1"], "--max_violations goes with"),
                (["--consistency_abs", "0.1"], "--consistency_abs goes with"),
                (["--consistency_rel", "0.1"], "--consistency_rel goes with"),
                (K + ["--with_consistency_check"], "exclude each other"),
                (K + ["--consistency_abs", "inf"], "--consistency_abs takes")]),
            (filter_depth_maps, ["scene", "predictions", str(tmp_path / "filtered")], [
                (["--max_violations", "-1"], "--max_violations takes"),
                (["--consistency_rel", "-1"], "--consistency_rel takes"),
                (["--border", "-1"], "--border"), (["--start_end", "3"], "--start_end")])]:
        for argv, message in cases:
            with pytest.raises(SystemExit) as e:
                script.main(head + argv)
            assert e.value.code == 2, argv
            assert message in capsys.readouterr().err, argv
    assert os.listdir(str(tmp_path)) == []
    a = filter_depth_maps.build_parser().parse_args(["s", "p", "f"])
    assert a.min_consistent_views is None and a.border == 0.0 and a.pred_suffix == "depth"


# ------------------------------------------------------------------------------ on the GPU
H, W, SCALE = 36, 64, 20.0
PATCH = (slice(14, 18), slice(30, 36))          # frame 0: a floater at 0.8 of the depth


def _mock_cameras(n):
    """The first n cameras of the mock scene for images of 1280 / 20 x 720 / 20."""
    from raynet_amd.common.camera import Camera
    from raynet_amd.common.scene import read_krt
    cams = []
    for name in sorted(os.listdir(os.path.join(MOCK, "cams_krt")))[:n]:
        K, R, t = read_krt(os.path.join(MOCK, "cams_krt", name))
        K = np.array(K, D)
        K[:2] /= SCALE
        cams.append(Camera(K, R, t))
    return cams


def _ground_depth(cam, z0=0.0):
    """(H, W) float32: the distance from the camera centre to the plane z = z0 along every
    pixel's ray, 0 where the ray does not meet it."""
    K, R = np.asarray(cam.K, D), np.asarray(cam.R, D)
    c = -R.T @ np.asarray(cam.t, D).reshape(3)
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    d = np.stack([X, Y, np.ones_like(X)], -1) @ np.linalg.inv(K).T @ R
    with np.errstate(all="ignore"):
        steps = (z0 - c[2]) / d[..., 2]
        depth = steps * np.sqrt((d * d).sum(-1))
    return np.where(np.isfinite(depth) & (steps > 0), depth, 0.0).astype(F)


@pytest.mark.gpu
def test_filter_depth_maps_writes_the_truths_counts(tmp_path, capsys):
    from mesh_harness import write_restrepo_scene
    from raynet_amd.common.scene import get_scene, parse_scene_info
    from raynet_amd.scripts import convert_to_pointcloud, filter_depth_maps, fuse_depth_maps
    cams = _mock_cameras(4)
    bbox = np.asarray(parse_scene_info(os.path.join(MOCK, "scene_info.xml")), F).reshape(-1)
    maps = [_ground_depth(c) for c in cams]
    assert all((m > 0).mean() > 0.9 for m in maps)
    maps[0][PATCH] = (maps[0][PATCH] * F(0.8)).astype(F)
    scene_dir, preds, out = str(tmp_path / "scene"), str(tmp_path / "preds"), str(tmp_path / "out")
    write_restrepo_scene(scene_dir, bbox, cams, H, W, maps)
    os.makedirs(preds)
    for i, m in enumerate(maps):
        np.save(os.path.join(preds, "depth_%03d.npy" % i), m)
    # (half a pixel of this slanted ground is up to 0.15 of depth: the tolerance exceeds it)
    flags = ["--consistency_abs", "0.3", "--consistency_rel", "0.005"]
    assert filter_depth_maps.main([scene_dir, preds, out, "--start_end", "0,4"] + flags) == 0
    printed = capsys.readouterr().out
    assert sorted(os.listdir(out)) == sorted(
        "%s_%03d.npy" % (name, i) for name in ("agree", "depth", "violate") for i in range(4))
    # the truth, from the scene as the script read it (its cameras are the text's)
    scene = get_scene("restrepo", scene_dir)
    read = [scene.get_image(i).camera for i in range(4)]
    rows, depths = ct.pack_cameras(read), np.stack(maps)
    at_ = np.arange(W)[None, :] * H + np.arange(H)[:, None]
    total_dropped = 0
    for i, cam in enumerate(read):
        points = et.depth_points(H, W, cam.P_pinv, np.asarray(cam.center, D).reshape(4), maps[i])
        _, agree, violate, _ = [w[at_] for w in
                                ct.check_points(points, rows, depths, i, 0.3, 0.005, 0.0)]
        got_agree = np.load(os.path.join(out, "agree_%03d.npy" % i))
        got_violate = np.load(os.path.join(out, "violate_%03d.npy" % i))
        got_depth = np.load(os.path.join(out, "depth_%03d.npy" % i))
        assert got_agree.dtype == got_violate.dtype == np.uint8 and got_depth.dtype == F
        assert got_agree.shape == got_violate.shape == got_depth.shape == (H, W)
        assert np.array_equal(got_agree, ct.popcount(agree))
        assert np.array_equal(got_violate, ct.popcount(violate))
        keep = ct.keep(maps[i], agree, violate, 2, 0)
        assert np.array_equal(got_depth.view(np.uint32), np.where(keep, maps[i], F(0)).view(np.uint32))
        measured = maps[i] > 0
        violating = measured & (ct.popcount(violate) > 0)
        disagreeing = measured & ~violating & (ct.popcount(agree) < 2)
        line = "frame %d: %d of %d measured pixels dropped, %d disagreeing and %d violating" % (
            i, int((measured & ~keep).sum()), int(measured.sum()), int(disagreeing.sum()),
            int(violating.sum()))
        assert line in printed, (line, printed)
        total_dropped += int((measured & ~keep).sum())
        if i == 0:
            assert (got_violate[PATCH] >= 1).all() and (got_depth[PATCH] == 0).all()
            outside = np.ones((H, W), bool)
            outside[PATCH] = False
            assert not got_violate[outside].any()
    assert total_dropped >= 24
    # the other scripts take the flags: the fused mesh is that of the filtered maps, and the cloud
    # has a point per kept pixel
    common = ["--start_end", "0,4", "--grid_shape", "20,20,8"]
    checked, direct = str(tmp_path / "checked.ply"), str(tmp_path / "direct.ply")
    assert fuse_depth_maps.main([scene_dir, preds, checked, "--min_consistent_views", "2"] + flags
                                + common) == 0
    assert "frame 0: " in capsys.readouterr().out
    assert fuse_depth_maps.main([scene_dir, out, direct] + common) == 0
    assert open(checked, "rb").read() == open(direct, "rb").read()
    plain = str(tmp_path / "plain.ply")
    assert fuse_depth_maps.main([scene_dir, preds, plain] + common) == 0
    assert "frame 0: " not in capsys.readouterr().out
    assert open(plain, "rb").read() != open(checked, "rb").read()
    cloud = ["--frame_idxs", ":4", "--borders", "2"]
    kept, _ = convert_to_pointcloud.main([scene_dir, preds, str(tmp_path / "c1"),
                                          "--min_consistent_views", "2"] + flags + cloud)
    assert "frame 3: " in capsys.readouterr().out
    every, _ = convert_to_pointcloud.main([scene_dir, preds, str(tmp_path / "c3")] + cloud)
    # the script selects the pixels where the scene's own map (these maps) is not 0, inside the
    # borders, row by row; the kept ones among them, in that order
    sl = (slice(2, H - 2), slice(2, W - 2))
    among = np.concatenate([np.load(os.path.join(out, "depth_%03d.npy" % i))[sl][maps[i][sl] != 0] != 0
                            for i in range(4)])
    assert every.shape == (3, len(among)) and 0 < among.sum() < len(among)
    assert kept.shape == (3, int(among.sum())) and np.array_equal(kept, every[:, among])
