"""The flags of raynet/scripts/arguments.py that reach the training code of this package, with
the reference's names and defaults, and what the two training scripts share."""
import json

import numpy as np

from .scene_flags import ints as _ints


def _floats(x):
    return tuple(map(float, x.split(",")))


SAMPLING_POLICIES = ["sample_in_bbox", "sample_in_range", "sample_in_disparity"]


def add_nn_arguments(p):
    # arguments.py:8-95
    p.add_argument("--lr", type=float, default=1e-3, help="Learning rate (default 1e-3)")
    p.add_argument("--reducer", choices=["average"], default="average")
    p.add_argument("--merge_layer", choices=["dot-product"], default="dot-product")
    p.add_argument("--optimizer", choices=["Adam", "SGD"], default="Adam")
    p.add_argument("--momentum", type=float, default=0.9, help="SGD momentum (default=0.9)")
    # (the reference's default names a Keras wrapper its end-to-end script then refuses; the
    # twin is the one architecture here under both names)
    p.add_argument("--network_architecture", choices=["simple_cnn", "simple_nn_for_training"],
                   default="simple_nn_for_training")
    p.add_argument("--cnn_factory", choices=["simple_cnn"], default="simple_cnn")
    p.add_argument("--loss", choices=["categorical_crossentropy", "emd", "squared_emd",
                                      "expected_squared_error"], default="emd")
    p.add_argument("--padding", default=None, type=int, help="Zero padding around images")
    p.add_argument("--weight_decay", type=float, default=0.0,
                   help="L2 regularizer factor on the convolution kernels")


def add_training_arguments(p):
    # arguments.py:98-138
    p.add_argument("--epochs", type=int, default=500)
    p.add_argument("--steps_per_epoch", type=int, default=500)
    p.add_argument("--n_test_samples", type=int, default=500,
                   help="Number of samples used in the validation set (default=500)")


def add_generation_arguments(p):
    # arguments.py:141-224
    p.add_argument("--patch_shape", type=_ints, default="11,11,3")
    p.add_argument("--depth_planes", type=int, default=32)
    p.add_argument("--neighbors", type=int, default=4)
    p.add_argument("--target_distribution_factory", choices=["dirac", "guassian"], default="dirac")
    p.add_argument("--stddev_factor", type=float, default=1.0)
    p.add_argument("--std_is_distance", action="store_true")
    p.add_argument("--sampling_policy", choices=SAMPLING_POLICIES, default="sample_in_bbox",
                   help="Where on the viewing ray the depth planes lie (default=sample_in_bbox)")
    p.add_argument("--depth_range", type=_floats, default="3.0,7.0",
                   help="The depth range used when sampling planes in range")
    p.add_argument("--grid_shape", type=_ints, default="256,256,128")
    p.add_argument("--maximum_number_of_marched_voxels", type=int, default=650)


def add_dataset_related_arguments(p):
    # arguments.py:300-330
    p.add_argument("--select_neighbors_based_on", choices=["filesystem", "distance"],
                   default="filesystem")
    p.add_argument("--illumination_condition",
                   choices=["max"] + ["%d_r5000" % i for i in range(7)], default="max")
    p.add_argument("--dataset_type", choices=["restrepo", "dtu"], default="restrepo")


def add_run_arguments(p):
    """Not the reference's: reproducibility and restarts."""
    p.add_argument("--resume", action="store_true",
                   help="Continue from the newest state.%%d.pt of the output directory")
    p.add_argument("--bp_iterations", type=int, default=3)


def generation_parameters(args):
    """GenerationParameters.from_options, plus what it leaves out: the target distribution
    factory the flags name, and the grid as the int32 array the kernels' callers expect."""
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.train_network.targets import get_target_distribution_factory
    if isinstance(getattr(args, "depth_range", None), str):      # (argparse leaves a default as it is)
        args.depth_range = _floats(args.depth_range)
    gp = GenerationParameters.from_options(args)
    gp.grid_shape = np.array(args.grid_shape, np.int32)
    gp.target_distribution_factory = get_target_distribution_factory(
        args.target_distribution_factory, args.stddev_factor, args.std_is_distance)
    return gp


def scenes_split(path):
    """{"train": [...], "test": [...]} scene indices (the reference's train_test_scenes_range)."""
    with open(path) as f:
        split = json.load(f)
    return tuple(split["train"]), tuple(split["test"])


def datasets(args, test_directory):
    from raynet_amd.common.dataset import build_dataset
    return (build_dataset(args.dataset_type, args.training_directory, args.illumination_condition,
                          args.select_neighbors_based_on),
            build_dataset(args.dataset_type, test_directory, args.illumination_condition,
                          args.select_neighbors_based_on))


def seed_everything(seed):
    import torch
    np.random.seed(seed)
    torch.manual_seed(seed)
