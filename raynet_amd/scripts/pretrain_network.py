#!/usr/bin/env python3
"""Pre-training of the MV-CNN on depth-space targets: the reference's `raynet_pretrain`
(raynet/scripts/pretrain_network.py) on MI355X.

    python -m raynet_amd.scripts.pretrain_network TRAIN_DIR TEST_DIR OUT_DIR SPLIT.json \\
        --dataset_type restrepo --grid_shape 64,64,32 --maximum_number_of_marched_voxels 160 \\
        --target_distribution_factory guassian --stddev_factor 2.0

A sample is a ray: the patches around its D sample points in the reference view and its
neighbours, and the target distribution of its ground-truth point over those points
(train_network/targets.py).  --epochs x --steps_per_epoch steps of --batch_size rays (or
--iterations steps) with batch statistics in the batch normalisation; a validation in inference
mode and a snapshot every epoch (--validate_every / --snapshot_every steps).  Writes
OUT_DIR/train_statistics.txt, val_loss.txt, weights.%d.npz -- the weight_file of
scripts/train_raynet.py and scripts/forward_pass.py -- and state.%d.pt for --resume.
"""
import argparse
import sys

from raynet_amd.scripts import training_arguments as ta


def build_parser():
    p = argparse.ArgumentParser(description=("Train a network to predict the per-pixel depth value "
                                             "for an image given a set of images from different views"))
    p.add_argument("training_directory", help="Path to the folder containing the training set")
    p.add_argument("test_directory", help="Path to the folder containing the test set")
    p.add_argument("output_directory", help="Save the output files in that directory")
    p.add_argument("train_test_scenes_range",
                   help="Path to the file containing the train-test splits")
    p.add_argument("--weight_file", help="An initial weights file")
    p.add_argument("--batch_size", type=int, default=32, help="Number of samples in a batch")
    p.add_argument("--seed", type=int, default=0, help="Seed for the PRNG")
    p.add_argument("--iterations", type=int, default=None,
                   help="Number of updates (default: epochs x steps_per_epoch)")
    p.add_argument("--validate_every", type=int, default=None,
                   help="Validate every so many updates (default: steps_per_epoch)")
    p.add_argument("--snapshot_every", type=int, default=None,
                   help="Save the weights every so many updates (default: steps_per_epoch)")
    p.add_argument("--repeat_from_same_scene", type=int, default=1000,
                   help="Samples drawn from a scene before another one is chosen")
    ta.add_training_arguments(p)
    ta.add_nn_arguments(p)
    ta.add_generation_arguments(p)
    ta.add_dataset_related_arguments(p)
    ta.add_run_arguments(p)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    from raynet_amd.scripts.forward_pass import load_model
    from raynet_amd.train_network.ray_sampler import RayBatchSampler, SceneBank
    from raynet_amd.train_network.trainer import Trainer, draw_validation_set
    if args.loss == "expected_squared_error":
        raise ValueError("expected_squared_error is a voxel-space loss: end-to-end training only")
    ta.seed_everything(args.seed)
    gp = ta.generation_parameters(args)
    training_dataset, test_dataset = ta.datasets(args, args.test_directory)
    train_scenes, test_scenes = ta.scenes_split(args.train_test_scenes_range)
    model = load_model(args.weight_file, "simple_cnn", in_channels=args.patch_shape[2])
    train_sampler = RayBatchSampler(SceneBank(training_dataset, gp), args.batch_size,
                                    mode="pretrain", scenes_range=train_scenes, seed=args.seed,
                                    repeat_from_same_scene=args.repeat_from_same_scene)
    test_sampler = RayBatchSampler(SceneBank(test_dataset, gp),
                                   min(args.batch_size, args.n_test_samples), mode="pretrain",
                                   scenes_range=test_scenes, seed=args.seed + 1,
                                   repeat_from_same_scene=args.repeat_from_same_scene)
    validation = draw_validation_set(test_sampler, args.n_test_samples)
    iterations = args.iterations if args.iterations is not None else args.epochs * args.steps_per_epoch
    trainer = Trainer(model, "pretrain", args.neighbors + 1, args.output_directory, loss=args.loss,
                      optimizer=args.optimizer, lr=args.lr, momentum=args.momentum,
                      weight_decay=args.weight_decay,
                      target_distribution_factory=gp.target_distribution_factory)
    trainer.fit(train_sampler, validation, iterations,
                args.validate_every or args.steps_per_epoch,
                args.snapshot_every or args.steps_per_epoch, resume=args.resume, log=print)
    return trainer


if __name__ == "__main__":
    main(sys.argv[1:])
