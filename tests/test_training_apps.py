"""The host side of the training applications: dataset discovery (common/dataset.py), the two
scripts' parsers against the reference's defaults, the split file, the sampler's schedules.  CPU."""
import json
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN


def _restrepo_tree(root, names, views=3):
    """Scene directories with PNGs written here, the golden cams_krt / scene_info.xml and depth
    maps."""
    from PIL import Image
    src = os.path.join(GOLDEN, "restrepo_mock_scene_1")
    cams = sorted(os.listdir(os.path.join(src, "cams_krt")))[:views]
    for k, name in enumerate(names):
        d = os.path.join(root, name)
        for sub in ("imgs", "cams_krt", "gt"):
            os.makedirs(os.path.join(d, sub))
        shutil.copy(os.path.join(src, "scene_info.xml"), d)
        for i, c in enumerate(cams):
            shutil.copy(os.path.join(src, "cams_krt", c), os.path.join(d, "cams_krt", c))
            Image.fromarray(np.full((6, 8, 3), 10 * k + i, np.uint8)).save(
                os.path.join(d, "imgs", "img_%02d.png" % i))
            np.save(os.path.join(d, "gt", "gt_depth_%d.npy" % i), np.full((6, 8), k + 1.0, np.float32))


def test_restrepo_dataset_orders_scenes_alphabetically_and_caches(tmp_path):
    from raynet_amd.common.dataset import RestrepoDataset, build_dataset
    from raynet_amd.common.scene import RestrepoScene
    names = ["zeta", "alpha", "Mid", "beta"]
    _restrepo_tree(str(tmp_path), names)
    ds = build_dataset("restrepo", str(tmp_path), "max", "filesystem")
    assert isinstance(ds, RestrepoDataset) and ds.n_scenes == 4
    assert ds.scenes == sorted(names)
    for i, name in enumerate(sorted(names)):
        s = ds.get_scene(i)
        assert isinstance(s, RestrepoScene) and s.n_images == 3
        k = names.index(name)
        assert s.get_image(1).image[0, 0, 0] == np.float32(10 * k + 1) / np.float32(255)
        assert float(s.get_depth_map(2)[0, 0]) == k + 1.0
        assert ds.get_scene(i) is s                         # built once
    with pytest.raises(ValueError):
        ds.get_scene(4)
    assert build_dataset("Restrepo", str(tmp_path), "max", "distance")._select_neighbors_based_on == "distance"


def test_dtu_dataset_counts_scans_and_keeps_two(tmp_path, monkeypatch):
    from raynet_amd.common import dataset as D
    for scan in (1, 4, 9):
        os.makedirs(os.path.join(str(tmp_path), "Rectified", "scan%03d" % scan))
    built = []

    class FakeScene(object):
        def __init__(self, base, idx, illumination, select_neighbors_based_on):
            built.append((idx, illumination, select_neighbors_based_on))
    monkeypatch.setattr(D, "DTUScene", FakeScene)
    ds = D.build_dataset("dtu", str(tmp_path), "3_r5000", "distance")
    assert isinstance(ds, D.DTUDataset) and ds.n_scenes == 3
    a = ds.get_scene(4)
    assert ds.get_scene(4) is a and built == [(4, "3_r5000", "distance")]
    ds.get_scene(9)
    ds.get_scene(1)                                       # evicts the least recently used: 4
    assert len(ds._cache) == 2 and 4 not in ds._cache
    assert ds.get_scene(4) is not a


@pytest.mark.parametrize("script", ["train_raynet", "pretrain_network"])
def test_parser_defaults_are_the_references(script):
    import importlib
    ref = json.load(open(os.path.join(GOLDEN, "ref_training_parser_defaults.json")))
    mod = importlib.import_module("raynet_amd.scripts." + script)
    positionals = ref[script + "_positionals"]
    args = vars(mod.build_parser().parse_args(["x%d" % i for i in range(len(positionals))]))
    for i, name in enumerate(positionals):
        assert args[name] == "x%d" % i
    for name, want in ref[script].items():
        got = args[name]
        assert (list(got) if isinstance(got, tuple) else got) == want, (name, got, want)
    # what this package adds keeps out of the way
    assert args["resume"] is False and args["seed"] == 0
    if script == "train_raynet":
        assert args["batch_norm"] == "frozen"
        with pytest.raises(ValueError, match="simple_cnn"):     # as the reference: say it
            mod.main(["a", "b", "c", "d", "e"])


def test_split_file_and_schedules(tmp_path):
    from raynet_amd.scripts.training_arguments import scenes_split
    from raynet_amd.train_network.ray_sampler import RayBatchSampler
    path = os.path.join(str(tmp_path), "split.json")
    json.dump({"train": [3, 5, 6], "test": [1]}, open(path, "w"))
    train, test = scenes_split(path)
    assert train == (3, 5, 6) and test == (1,)

    class Bank(object):
        class dataset(object):
            n_scenes = 8

        class gp(object):
            patch_shape = (11, 11, 3)
    V = 12
    s = RayBatchSampler(Bank, 100, mode="random", scenes_range=train, n_rays=200, window=4, seed=1)
    seen = set()
    for _ in range(200):
        assert s._view_range(V) == (2, V - 4)
        seen.add(s.scenes_range[s._scene_pos])
        s._advance(V, 100)
    assert seen == {3, 5, 6}                              # only the split's scenes, all of them
    w = RayBatchSampler(Bank, 100, mode="window", scenes_range=train, n_rays=200, window=4, seed=1)
    walk = []
    for _ in range(20):
        walk.append((w.scenes_range[w._scene_pos], w._view_range(V)))
        w._advance(V, 100)
    # start advances by 2 every n_rays rays; at V - window the next scene starts at 2
    assert walk[:8] == [(3, (2, 6)), (3, (2, 6)), (3, (4, 8)), (3, (4, 8)), (3, (6, 10)),
                        (3, (6, 10)), (5, (2, 6)), (5, (2, 6))]
    assert walk[18][0] == 3
    p = RayBatchSampler(Bank, 100, mode="pretrain", scenes_range=test, repeat_from_same_scene=150)
    assert p._view_range(V) == (2, V) and p.patch_shape == (11, 11)
    with pytest.raises(ValueError):
        RayBatchSampler(Bank, 100, mode="random", window=4)._view_range(6)
    with pytest.raises(ValueError):
        RayBatchSampler(Bank, 100, mode="other")


def test_generation_parameters_get_the_target_factory_after_from_options():
    from raynet_amd.scripts import pretrain_network
    from raynet_amd.scripts.training_arguments import generation_parameters
    from raynet_amd.train_network.targets import dirac_distribution
    args = pretrain_network.build_parser().parse_args(["a", "b", "c", "d", "--grid_shape", "8,8,4"])
    gp = generation_parameters(args)
    assert gp.target_distribution_factory is dirac_distribution
    assert gp.grid_shape.dtype == np.int32 and list(gp.grid_shape) == [8, 8, 4]
    assert gp.padding == 11 and gp.depth_planes == 32 and gp.max_number_of_marched_voxels == 650
    args = pretrain_network.build_parser().parse_args(
        ["a", "b", "c", "d", "--target_distribution_factory", "guassian", "--std_is_distance"])
    assert generation_parameters(args).target_distribution_factory.__name__ == "inner"
