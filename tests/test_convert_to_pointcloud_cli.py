"""Host side of scripts/convert_to_pointcloud.py: the reference's flags and defaults
(raynet/scripts/convert_to_pointcloud.py:38-75, arguments.py:259-330), its file-name format
search and its filter factory; compute_metrics.run takes a factory."""
import inspect
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN


def test_parser_mirrors_the_reference_flags_and_defaults():
    from raynet_amd.scripts import convert_to_pointcloud as cp
    a = cp.build_parser().parse_args(["data", "preds", "out"])
    assert (a.dataset_directory, a.predictions_directory, a.output_directory) == \
        ("data", "preds", "out")
    assert a.scene_idx == 0 and a.frame_idxs == slice(None, None) and a.pred_suffix == "depth"
    assert a.select_neighbors_based_on == "filesystem" and a.illumination_condition == "max"
    assert a.dataset_type == "restrepo"
    assert a.borders == 40 and a.truncate == float("inf") and a.min_distance == -1
    assert a.consistency_threshold == 0.75 and a.n_neighbors == 5
    assert a.with_consistency_check is False and a.seed == 0
    a = cp.build_parser().parse_args(
        ["d", "p", "o", "--min_distance", "0.2", "--seed", "4", "--frame_idxs", "1,3",
         "--scene_idx", "9", "--pred_suffix", "gt_depth", "--dataset_type", "dtu",
         "--with_consistency_check", "--borders", "3", "--n_neighbors", "2",
         "--consistency_threshold", "0.5"])
    assert a.min_distance == 0.2 and a.seed == 4 and a.frame_idxs == [1, 3] and a.scene_idx == 9
    assert a.pred_suffix == "gt_depth" and a.dataset_type == "dtu" and a.with_consistency_check
    assert (a.borders, a.n_neighbors, a.consistency_threshold) == (3, 2, 0.5)
    with pytest.raises(SystemExit):
        cp.build_parser().parse_args(["data", "preds"])            # the output directory
    assert callable(cp.run) and callable(cp.main)


def test_find_format(tmp_path):
    from raynet_amd.scripts.convert_to_pointcloud import find_format
    d = str(tmp_path)
    assert find_format(d, "depth", 7) == "depth_%03d.npy"          # nothing there: the padded one
    np.save(os.path.join(d, "depth_007.npy"), np.zeros(1))
    assert find_format(d, "depth", 7) == "depth_%03d.npy"
    np.save(os.path.join(d, "depth_7.npy"), np.zeros(1))
    assert find_format(d, "depth", 7) == "depth_%d.npy"
    assert find_format(d, "gt_depth", 7) == "gt_depth_%03d.npy"
    assert find_format(d, "depth", 7) % (12,) == "depth_12.npy"


class _MaskedScene(object):
    bbox = np.array([[0, 0, 0, 1, 2, 3]], np.float32)
    observation_mask = np.ones((4, 5, 6), np.uint8)


def test_build_filter_factory(tmp_path):
    from raynet_amd import metrics
    from raynet_amd.common.scene import RestrepoScene
    from raynet_amd.scripts.convert_to_pointcloud import build_filter_factory
    # (the mock scene ships cameras and the bounding box only: an empty imgs/ next to a copy)
    shutil.copytree(os.path.join(GOLDEN, "restrepo_mock_scene_1"), str(tmp_path / "scene"))
    os.makedirs(str(tmp_path / "scene" / "imgs"))
    restrepo = RestrepoScene(str(tmp_path / "scene"))
    assert restrepo.observation_mask is None
    ff = build_filter_factory(restrepo, -1)
    assert isinstance(ff, metrics.FiltersFactory) and not ff.has_filters and ff.filters == []
    ff = build_filter_factory(restrepo, 0.5, str(tmp_path), seed=3)
    assert [type(f) for f in ff.filters] == [metrics.ReduceDensity]
    assert ff.filters[0].seed == 3 and ff.filters[0].output_directory == str(tmp_path)
    ff = build_filter_factory(_MaskedScene(), 0.25, "somewhere", seed=2)
    assert [type(f) for f in ff.filters] == [metrics.VoxelMask, metrics.ReduceDensity]
    assert all(f.output_directory == "somewhere" for f in ff.filters) and ff.filters[1].seed == 2
    ff = build_filter_factory(_MaskedScene(), -1)
    assert [type(f) for f in ff.filters] == [metrics.VoxelMask]
    assert ff.filters[0].output_directory is None
    with pytest.raises(ValueError):
        build_filter_factory(restrepo, 0)


def test_compute_metrics_takes_a_filter_factory():
    from raynet_amd import metrics
    from raynet_amd.scripts import compute_metrics as cm
    assert inspect.signature(cm.run).parameters["filter_factory"].default is None
    a = cm.build_parser().parse_args(["d", "p", "accuracy"])
    ff = metrics.FiltersFactory([metrics.ReduceDensity(0.5)])
    for name in ("accuracy", "completeness", "surface_accuracy", "surface_completeness"):
        assert cm.build_metric(name, a, ff).filter_factory is ff
        assert not cm.build_metric(name, a).filter_factory.has_filters
    assert "convert_to_pointcloud" in cm.__doc__
