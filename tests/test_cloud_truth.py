"""The semantics of the cloud z-buffer and its hidden-point filter on
the NumPy restatement tests/cloud_truth.py, and the host-side parts of the DTU fallback and the
command-line tool that need no GPU."""
import numpy as np
import pytest

import cloud_truth as truth
from dtu_tree import write_dtu_tree

F = np.float32


def _frontal_rows(H, W, focal):
    """One camera at the origin looking along +z."""
    K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1.0]])
    return np.concatenate([K.ravel(), np.eye(3).ravel(), np.zeros(3)]).reshape(1, 21)


def _sheet(us, vs, z, H, W, focal):
    """Points at depth z (array or scalar) that project to pixel coordinates (us, vs)."""
    z = np.broadcast_to(np.asarray(z, np.float64), us.shape)
    return np.stack([(us - W / 2.0) / focal * z, (vs - H / 2.0) / focal * z, z], axis=-1)


def test_zbuffer_rounds_half_to_even_and_keeps_the_nearest():
    H, W, focal = 8, 12, 16.0                   # W/2, H/2 and 1/16 steps: exact in fp32
    rows = _frontal_rows(H, W, focal)
    us = np.array([2.5, 3.5, 7.0, 7.0, -0.5, 11.5, 5.0, 5.0])
    vs = np.array([1.0, 1.0, 2.5, 3.5, 4.0, 4.0, -0.5, 7.5])
    pts = _sheet(us, vs, 2.0, H, W, focal)
    pts = np.concatenate([pts, _sheet(np.array([2.0]), np.array([1.0]), 1.5, H, W, focal)])
    z = truth.zbuffer(pts, rows, H, W)[0]
    filled = {(int(v), int(u)): float(z[v, u]) for v, u in zip(*np.nonzero(np.isfinite(z)))}
    # 2.5 -> 2 (and the nearer point wins there), 3.5 -> 4, -0.5 -> 0, 11.5 -> 12 = W: outside,
    # 7.5 -> 8 = H: outside
    assert filled == {(1, 2): 1.5, (1, 4): 2.0, (2, 7): 2.0, (4, 7): 2.0, (4, 0): 2.0, (0, 5): 2.0}


def test_zbuffer_drops_points_behind_the_camera_and_non_finite_ones():
    H, W, focal = 8, 12, 16.0
    rows = _frontal_rows(H, W, focal)
    pts = np.array([[0, 0, -1.0], [0, 0, 0.0], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.inf],
                    [0, 0, -np.inf]], F)
    assert not np.isfinite(truth.zbuffer(pts, rows, H, W)).any()
    assert truth.zbuffer(np.zeros((0, 3), F), rows, H, W).shape == (1, H, W)


def _two_sheets(H, W, focal):
    """A front sheet (z = 2) with gaps -- a 1.4-pixel lattice over the middle of the image --
    in front of a dense back sheet (z = 3, a 0.5-pixel lattice over the whole image)."""
    fu, fv = np.meshgrid(np.arange(10.0, W - 10.0, 1.4), np.arange(10.0, H - 10.0, 1.4))
    bu, bv = np.meshgrid(np.arange(0.0, W - 0.75, 0.5), np.arange(0.0, H - 0.75, 0.5))
    return (_sheet(fu.ravel(), fv.ravel(), 2.0, H, W, focal),
            _sheet(bu.ravel(), bv.ravel(), 3.0, H, W, focal))


def test_filter_removes_the_back_sheet_behind_a_front_sheet():
    H, W, focal = 48, 64, 60.0
    rows = _frontal_rows(H, W, focal)
    front, back = _two_sheets(H, W, focal)
    pts = np.concatenate([front, back]).astype(F)
    raw = truth.zbuffer(pts, rows, H, W)[0]
    out = truth.depth_maps(pts, rows, H, W)[0]
    inner = (slice(11, H - 12), slice(11, W - 12))          # the front sheet's extent
    assert (raw[inner] == 3.0).sum() > 0.3 * raw[inner].size       # the back shows through
    assert (raw[inner] == 2.0).sum() > 0.3 * raw[inner].size
    assert not (out[inner] == 3.0).any()                           # ... and is gone
    assert np.array_equal(out == 2.0, raw == 2.0)                  # the front stays, all of it
    # away from the front sheet the back sheet is the surface and stays
    assert (out[:8] == 3.0).all() and (out[:, :8] == 3.0).all()


def _tilted_sheet(H, W, focal, rng):
    """A plane tilted 60 degrees against the image plane (about the image's vertical axis),
    sampled at 0.6 x 0.6 pixel footprints on the surface with jitter: 0.3 x 0.6 pixels in the
    image, more than five points per pixel."""
    z0 = 4.0
    step = 0.6 * z0 / focal
    s, t = np.meshgrid(np.arange(-1.2, 1.2, step), np.arange(-1.0, 1.0, step))
    s = s + rng.uniform(-0.5, 0.5, s.shape) * step
    t = t + rng.uniform(-0.5, 0.5, t.shape) * step
    c, sn = np.cos(np.pi / 3), np.sin(np.pi / 3)
    return np.stack([s * c, t, z0 + s * sn], axis=-1).reshape(-1, 3).astype(F)


def test_filter_keeps_a_slanted_surface_where_a_fixed_tolerance_deletes_it():
    H, W, focal = 48, 64, 60.0
    rows = _frontal_rows(H, W, focal)
    pts = _tilted_sheet(H, W, focal, np.random.default_rng(0))
    raw = np.isfinite(truth.zbuffer(pts, rows, H, W)[0])
    # the sheet's interior: filled pixels whose 3 x 3 neighbours are all filled
    interior = raw.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior &= np.roll(np.roll(raw, dy, 0), dx, 1)
    interior[[0, -1]] = False
    interior[:, [0, -1]] = False
    n = int(interior.sum())
    assert n > 400
    lost = {}
    for gain in (1.5, 0.0):
        kept = truth.depth_maps(pts, rows, H, W, slope_gain=gain)[0] != 0
        lost[gain] = float((interior & ~kept).sum()) / n
    # measured: 1 of 531 interior pixels lost with the default filter (0.0019), 530 of 531 with
    # slope_gain = 0 (0.9981):
    # the depth changes by tan(60 deg) = 1.73 footprints per pixel, more than tau_px = 1
    print("interior pixels %d, lost: default %.4f, fixed tolerance %.4f" % (n, lost[1.5], lost[0.0]))
    assert lost[1.5] <= 0.10
    assert lost[0.0] >= 0.90
    assert lost[0.0] >= 9 * max(lost[1.5], 0.01)


def test_closing_radius_zero_returns_the_raw_buffer():
    H, W, focal = 48, 64, 60.0
    rows = _frontal_rows(H, W, focal)
    front, back = _two_sheets(H, W, focal)
    pts = np.concatenate([front, back]).astype(F)
    raw = truth.zbuffer(pts, rows, H, W)
    out = truth.depth_maps(pts, rows, H, W, closing_radius=0)
    assert np.array_equal(out, np.where(np.isfinite(raw), raw, F(0)))
    assert (out == 3.0).any() and (out == 2.0).any()


def test_window_min_is_a_plus_infinity_padded_minimum():
    rng = np.random.default_rng(1)
    z = rng.uniform(1, 2, (2, 7, 9)).astype(F)
    z[rng.random(z.shape) < 0.4] = np.inf
    for S in (1, 2):
        got = truth.window_min(z, S)
        for v, y, x in ((0, 0, 0), (1, 6, 8), (0, 3, 4), (1, 0, 5)):
            assert got[v, y, x] == z[v, max(0, y - S):y + S + 1, max(0, x - S):x + S + 1].min()


def test_dtu_scene_without_depth_files_or_cloud_names_both_paths(tmp_path):
    from raynet_amd.common.camera import Camera
    from raynet_amd.common.scene import DTUScene
    H, W = 6, 8
    cams = [Camera.look_at([1.0 + k, -2.0, 0.5], [0, 0, 0], 50.0, H, W) for k in range(2)]
    base = write_dtu_tree(tmp_path, cams, H, W, scan=7)
    s = DTUScene(base, 7)
    with pytest.raises(FileNotFoundError) as e:
        s.get_gt_depth_map(1)
    msg = str(e.value)
    assert "Depth/scan007" in msg.replace("\\", "/")
    assert "Points/stl/stl007_total.ply" in msg.replace("\\", "/")
    assert "frame 1" in msg
    with pytest.raises(FileNotFoundError):
        s.get_depth_map(0)


def test_dtu_scene_reads_depth_files_as_before(tmp_path):
    from raynet_amd.common.camera import Camera
    from raynet_amd.common.scene import DTUScene
    H, W = 6, 8
    cams = [Camera.look_at([1.0 + k, -2.0, 0.5], [0, 0, 0], 50.0, H, W) for k in range(2)]
    maps = [np.full((H, W), 2.0 + k, F) for k in range(2)]
    base = write_dtu_tree(tmp_path, cams, H, W, scan=7, depth_maps=maps)
    s = DTUScene(base, 7)
    for k in range(2):
        assert np.array_equal(s.get_gt_depth_map(k), maps[k])
    assert s._cloud_renderer is None


def test_cli_refuses_frames_in_dtu_mode(tmp_path):
    from raynet_amd.scripts import gt_depth_maps
    with pytest.raises(SystemExit) as e:
        gt_depth_maps.main([str(tmp_path), "--dataset_type", "dtu", "--scene_idx", "1",
                            "--frames", "0,1"])
    assert "--frames" in str(e.value) and "dtu" in str(e.value)
    with pytest.raises(SystemExit) as e:
        gt_depth_maps.main([str(tmp_path), "--dataset_type", "dtu"])
    assert "--scene_idx" in str(e.value)
