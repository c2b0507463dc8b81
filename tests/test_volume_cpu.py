"""The occupancy volume's host side (no GPU): the two entries in the header and the ctypes table,
the command lines' flags, OccupancyVolume's file and its voxel cloud."""
import os

import numpy as np
import pytest
import torch

import abi_header


@pytest.mark.parametrize("name,params", [
    ("rn_occupancy_grid", ["rn_ctx *ctx", "const float *acc", "int32_t bricked", "float bias",
                           "float *belief_out", "void *stream"]),
    ("rn_volume_render", ["rn_ctx *ctx", "int32_t n", "const float *ray_start",
                          "const float *ray_end", "const float *camera_center",
                          "const float *belief", "float *out", "int64_t out_stride",
                          "void *stream"]),
])
def test_entries_are_declared_and_bound_with_matching_arity(name, params):
    """(The types of every entry, these two included: tests/test_abi.py.)"""
    import ctypes
    from raynet_amd import _lib
    assert abi_header.prototype(name) == ("int", params)
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(params)
    assert hasattr(ctypes.CDLL(_lib.build()), name)


def test_forward_pass_parser_knows_save_occupancy():
    from raynet_amd.scripts import forward_pass
    p = forward_pass.build_parser()
    assert p.parse_args(["scene", "out"]).save_occupancy is False
    assert p.parse_args(["scene", "out", "--save_occupancy"]).save_occupancy is True


@pytest.mark.parametrize("factory", ["multi_view_cnn", "multi_view_cnn_voxel_space"])
def test_save_occupancy_is_refused_for_the_other_factories(factory, capsys):
    from raynet_amd.scripts import forward_pass
    with pytest.raises(SystemExit) as e:
        forward_pass.main(["scene", "out", "--save_occupancy", "--forward_pass_factory", factory])
    assert e.value.code == 2
    assert "--save_occupancy needs --forward_pass_factory raynet" in capsys.readouterr().err


def test_render_volume_parser_defaults():
    from raynet_amd.scripts import forward_pass, render_volume
    p = render_volume.build_parser()
    a = p.parse_args(["scene", "occupancy.npz", "out"])
    assert (a.dataset_directory, a.occupancy_file, a.output_directory) == \
        ("scene", "occupancy.npz", "out")
    assert a.plane == "depth" and a.ply is None and a.threshold == 0.5 and a.all_voxels is False
    # the dataset and indexing flags are the forward pass's, defaults included
    f = forward_pass.build_parser().parse_args(["scene", "out"])
    for flag in ("dataset_type", "scene_idx", "start_end", "skip_every",
                 "select_neighbors_based_on", "illumination_condition"):
        assert getattr(a, flag) == getattr(f, flag), flag
    assert render_volume.PLANES == ["depth", "expected_depth", "median_depth"]
    for plane in render_volume.PLANES:
        assert p.parse_args(["s", "o.npz", "out", "--plane", plane]).plane == plane
    with pytest.raises(SystemExit):
        p.parse_args(["s", "o.npz", "out", "--plane", "opacity"])
    a = p.parse_args(["s", "o.npz", "out", "--ply", "c.ply", "--threshold", "0.7", "--all_voxels",
                      "--start_end", "2,9", "--skip_every", "1", "--dataset_type", "dtu"])
    assert (a.ply, a.threshold, a.all_voxels, a.start_end, a.skip_every, a.dataset_type) == \
        ("c.ply", 0.7, True, (2, 9), 1, "dtu")


def test_save_and_load_round_trip_exactly(tmp_path):
    from raynet_amd.volume import OccupancyVolume
    rng = np.random.default_rng(5)
    belief = rng.uniform(1e-4, 1 - 1e-4, (5, 6, 7)).astype(np.float32)
    bbox = np.array([-0.8, -0.6, -0.4, 0.8, 0.6, 0.41], np.float32)
    v = OccupancyVolume(belief, bbox.reshape(1, 6), np.array([5, 6, 7], np.int64))
    path = str(tmp_path / "occupancy.npz")
    v.save(path)
    assert os.path.isfile(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["bbox", "belief", "grid_shape"]
        assert z["belief"].dtype == np.float32 and np.array_equal(z["belief"], belief)
        assert z["bbox"].dtype == np.float32 and np.array_equal(z["bbox"], bbox)
        assert z["grid_shape"].tolist() == [5, 6, 7]
    w = OccupancyVolume.load(path)
    assert np.array_equal(w.belief.numpy(), belief) and np.array_equal(w.bbox, bbox)
    assert w.grid_shape == (5, 6, 7)
    # a file with anything else in it is not an occupancy volume
    other = str(tmp_path / "other.npz")
    np.savez(other, belief=belief, bbox=bbox, grid_shape=np.array([5, 6, 7]), extra=np.zeros(1))
    with pytest.raises(ValueError):
        OccupancyVolume.load(other)
    with pytest.raises(ValueError):
        OccupancyVolume(belief, bbox, (5, 6, 8))


def _volume(belief):
    from raynet_amd.volume import OccupancyVolume
    return OccupancyVolume(torch.from_numpy(belief), (-1, -1, -1, 1, 1, 1), belief.shape)


def test_pointcloud_of_a_solid_block():
    from raynet_amd.pointcloud import Pointcloud
    belief = np.full((4, 4, 4), 0.1, np.float32)
    belief[1:3, 1:3, 1:3] = 0.9
    for surface_only in (True, False):
        pc = _volume(belief).pointcloud(0.5, surface_only=surface_only)
        assert isinstance(pc, Pointcloud)
        pts = np.asarray(pc.points)
        assert pts.shape == (3, 8)            # every voxel of a 2 x 2 x 2 block is surface
        # centres of the cells 1 and 2 of a [-1, 1] axis cut in four: -0.25 and 0.25
        assert sorted(set(np.round(pts.ravel(), 6).tolist())) == [-0.25, 0.25]
    # [gx][gy][gz] order
    assert pts[:, 0].tolist() == [-0.25, -0.25, -0.25] and pts[:, 1].tolist() == [-0.25, -0.25, 0.25]


def test_pointcloud_of_a_solid_grid():
    belief = np.full((4, 4, 4), 0.9, np.float32)
    assert np.asarray(_volume(belief).pointcloud().points).shape == (3, 56)     # 64 - 2^3 inside
    assert np.asarray(_volume(belief).pointcloud(surface_only=False).points).shape == (3, 64)
    # the threshold is inclusive, and nothing is occupied above it
    assert np.asarray(_volume(belief).pointcloud(0.9, False).points).shape == (3, 64)
    assert np.asarray(_volume(belief).pointcloud(0.95).points).shape == (3, 0)
    # a hole at an inner voxel: 63 occupied, and its three inner neighbours become surface
    belief[1, 1, 1] = 0.2
    assert np.asarray(_volume(belief).pointcloud().points).shape == (3, 59)
