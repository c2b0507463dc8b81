"""The two training applications end to end on a temporary two-scene Restrepo dataset of the
plane scene: scripts/train_raynet.py and scripts/pretrain_network.py through their `main`."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPE = ["--depth_planes", "8", "--grid_shape", "32,32,16", "--maximum_number_of_marched_voxels", "96",
         "--batch_size", "128", "--optimizer", "Adam", "--lr", "2e-3", "--n_test_samples", "256"]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    import training_tree
    return training_tree.write_dataset(str(tmp_path_factory.mktemp("training")), GOLDEN)


def _lines(path):
    return open(path).read().splitlines()


@pytest.fixture(scope="module")
def pretrained(dataset, tmp_path_factory):
    from raynet_amd.scripts import pretrain_network
    directory, split = dataset
    out = str(tmp_path_factory.mktemp("pretrain"))
    trainer = pretrain_network.main([directory, directory, out, split, "--iterations", "30",
                                     "--validate_every", "10", "--snapshot_every", "10",
                                     "--seed", "3"] + SHAPE)
    return trainer, out


def test_pretraining_lowers_the_loss_and_writes_loadable_weights(pretrained):
    trainer, out = pretrained
    stats = _lines(os.path.join(out, "train_statistics.txt"))
    assert stats[0] == "scene_idx max_img_idx loss gamma" and len(stats) == 31
    rows = np.array([ln.split() for ln in stats[1:]], np.float64)
    assert np.all(rows[:, 0] == 0)                       # the split's training scene
    assert np.all((rows[:, 1] >= 2) & (rows[:, 1] < 7)) and np.isfinite(rows[:, 2]).all()
    loss = rows[:, 2]
    print("pre-training loss: first 5 %s, last 5 %s" % (loss[:5], loss[-5:]))
    assert loss[-5:].mean() < loss[:5].mean(), (loss[:5], loss[-5:])
    assert len(_lines(os.path.join(out, "val_loss.txt"))) == 3
    # snapshots at steps 0, 10, 20 and the final one
    assert sorted(glob.glob(os.path.join(out, "weights.*.npz"))) == \
        [os.path.join(out, "weights.%d.npz" % i) for i in range(4)]
    w = np.load(os.path.join(out, "weights.3.npz"))
    assert len(w.files) == 30 and w["arr_0"].shape == (3, 3, 3, 32)
    # batch statistics were used: the moving averages moved off their initial 0 / 1
    assert np.abs(w["arr_4"]).max() > 0


def test_end_to_end_training(dataset, pretrained, tmp_path):
    import torch
    from raynet_amd.scripts import train_raynet
    from raynet_amd.scripts.forward_pass import load_model
    directory, split = dataset
    weight_file = os.path.join(pretrained[1], "weights.3.npz")      # raynet_pretrain's output
    argv = [directory, directory, str(tmp_path), weight_file, split,
            "--network_architecture", "simple_cnn", "--train_with_gamma", "--validate_every", "10",
            "--snapshot_every", "10", "--gamma_range", "1e-3,0.5", "--seed", "4", "--window", "1"] + SHAPE
    trainer = train_raynet.main(argv + ["--iterations", "30"])
    out = trainer.output_directory
    assert os.path.dirname(out) == str(tmp_path) and "gamma_(0.031, 0.001, 0.5)" in out
    stats = _lines(os.path.join(out, "train_statistics.txt"))
    assert stats[0] == "scene_idx max_img_idx loss gamma" and len(stats) == 31
    rows = np.array([ln.split() for ln in stats[1:]], np.float64)
    assert np.isfinite(rows).all() and np.all(rows[:, 0] == 0)
    assert np.all((rows[:, 3] >= 1e-3) & (rows[:, 3] <= 0.5)) and len(set(rows[:, 3])) > 1
    val = [float(v) for v in _lines(os.path.join(out, "val_loss.txt"))]
    print("end-to-end: validation %s, training first / last %g / %g" % (val, rows[0, 2], rows[-1, 2]))
    assert len(val) == 3 and val[-1] < val[0], val
    # frozen statistics: the moving averages are the weight file's
    start = np.load(weight_file)
    last = sorted(glob.glob(os.path.join(out, "weights.*.npz")),
                  key=lambda f: int(f.split(".")[-2]))[-1]
    assert last.endswith("weights.3.npz")
    end = np.load(last)
    assert np.array_equal(start["arr_4"], end["arr_4"]) and np.array_equal(start["arr_5"], end["arr_5"])
    assert not np.array_equal(start["arr_0"], end["arr_0"])
    # the snapshot is the trained model, to the bit, through the forward pass's own loader
    image = np.random.default_rng(0).random((1, 40, 48, 3)).astype(np.float32)
    loaded = load_model(last)
    trainer.model.patch_path = "auto"
    assert torch.equal(loaded.predict(image), trainer.model.predict(image))

    # --resume: continues at the saved step and appends
    resumed = train_raynet.main(argv + ["--iterations", "35", "--resume"])
    assert resumed.step == 35
    stats2 = _lines(os.path.join(out, "train_statistics.txt"))
    assert stats2[:31] == stats and len(stats2) == 36
    assert len(_lines(os.path.join(out, "val_loss.txt"))) == 4          # step 30 validates
    assert os.path.exists(os.path.join(out, "weights.5.npz"))          # step 30 and the final one
