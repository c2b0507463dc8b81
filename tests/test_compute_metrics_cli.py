"""Host side of scripts/compute_metrics.py and of the surface accessors: the reference's flags
and defaults (raynet/scripts/compute_metrics.py:56-104, arguments.py:259-330), the frame
selection, and which scenes have a ground-truth surface."""
import numpy as np
import pytest


def test_parser_mirrors_the_reference_flags_and_defaults():
    from raynet_amd.scripts import compute_metrics as cm
    a = cm.build_parser().parse_args(["data", "preds", "ppmde", "surface_accuracy"])
    assert a.dataset_directory == "data" and a.predictions_directory == "preds"
    assert a.metric == ["ppmde", "surface_accuracy"]
    assert a.output_directory == "/tmp/" and a.frame_idxs == slice(None, None)
    assert a.predicted_files_format == "depth_%03d.npy" and a.use_pc_from_depthmap is False
    assert a.dataset_type == "restrepo" and a.borders == 40 and a.truncate == float("inf")
    assert a.with_consistency_check is False and a.consistency_threshold == 0.75
    assert a.n_neighbors == 5 and a.seed == 0 and a.surface_samples == 1000000
    assert cm.METRICS == ["ppmde", "accuracy", "completeness", "surface_accuracy",
                          "surface_completeness"]
    with pytest.raises(SystemExit):
        cm.build_parser().parse_args(["data", "preds", "chamfer"])
    with pytest.raises(SystemExit):
        cm.build_parser().parse_args(["data", "preds", "accuracy", "--min_distance", "0.1"])
    assert "ReduceDensity" in cm.__doc__ and "VoxelMask" in cm.__doc__


def test_frame_idxs_type():
    from raynet_amd.scripts.compute_metrics import frame_idxs_type
    n = np.arange(12)
    assert list(n[frame_idxs_type(":")]) == list(range(12))
    assert list(n[frame_idxs_type("2:9:3")]) == [2, 5, 8]
    assert list(n[frame_idxs_type("1,4,7")]) == [1, 4, 7]
    assert list(n[frame_idxs_type("5")]) == [5]


def test_metrics_are_built_with_the_flags():
    from raynet_amd import metrics
    from raynet_amd.scripts import compute_metrics as cm
    a = cm.build_parser().parse_args(["d", "p", "accuracy", "--truncate", "2.5", "--borders", "7",
                                      "--surface_samples", "123", "--seed", "9"])
    m = cm.build_metric("surface_accuracy", a)
    assert isinstance(m, metrics.SurfaceAccuracy) and m.truncate == 2.5
    assert not m.filter_factory.has_filters
    m = cm.build_metric("surface_completeness", a)
    assert isinstance(m, metrics.SurfaceCompleteness)
    assert (m.n_samples, m.seed, m.truncate) == (123, 9, 2.5)
    m = cm.build_metric("accuracy", a)
    assert isinstance(m, metrics.Accuracy) and m.borders == 7 and m.truncate == 2.5
    assert isinstance(cm.build_metric("completeness", a), metrics.Completeness)
    assert cm.build_metric("ppmde", a).borders == 7
    # the defaults of the classes
    assert metrics.SurfaceAccuracy().truncate == float("inf")
    m = metrics.SurfaceCompleteness(10)
    assert m.seed == 0 and m.truncate == float("inf") and not m.filter_factory.has_filters


def test_only_a_scene_with_triangles_has_a_surface():
    from raynet_amd.common.scene import DTUScene, RestrepoScene, Scene
    with pytest.raises(NotImplementedError):
        Scene.get_surface(Scene.__new__(Scene))
    assert DTUScene.get_surface is Scene.get_surface          # a point cloud, no triangles
    assert RestrepoScene.get_surface is not Scene.get_surface
