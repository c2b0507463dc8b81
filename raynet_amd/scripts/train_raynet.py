#!/usr/bin/env python3
"""End-to-end training of RayNet: the reference's `raynet_train`
(raynet/scripts/train_raynet.py) on MI355X.

    python -m raynet_amd.scripts.train_raynet TRAIN_DIR TEST_DIR OUT_DIR WEIGHTS.npz SPLIT.json \\
        --network_architecture simple_cnn --dataset_type restrepo --grid_shape 64,64,32 \\
        --maximum_number_of_marched_voxels 160 --train_with_gamma

Batches of --batch_size rays of many reference views come from train_network/ray_sampler.py
("random" for training, "window" for the fixed validation set, as the reference), a step is
forward_backward_pass (MV-CNN twin, HIP MRF block forward and analytic backward) with per-tensor
gradient clipping at 0.1.  Writes OUT_DIR/<experiment tag>/train_statistics.txt, val_loss.txt and
weights.%d.npz (what scripts/forward_pass.py --weight_file loads) with state.%d.pt for --resume.
"""
import argparse
import os
import sys

from raynet_amd.scripts import training_arguments as ta


def experiment_tag(args):
    gamma = (args.initial_gamma,) + args.gamma_range if args.train_with_gamma else args.initial_gamma
    return "experiment_lr-%r_optimizer-%s_loss-%s_gamma_%r" % (args.lr, args.optimizer, args.loss, gamma)


def get_number_of_neighboring_rays_test_set(dataset_type, n_test_samples):
    # train_raynet.py:40-50
    return 25 if dataset_type == "dtu" else max(1, n_test_samples // 180)


def build_parser():
    p = argparse.ArgumentParser(description="Train the RayNet in an end-to-end fashion")
    p.add_argument("training_directory", help="Path to the folder containing the training set")
    p.add_argument("testing_directory", help="Path to the folder containing the test set")
    p.add_argument("output_directory", help="Save the output files in that directory")
    p.add_argument("weight_file", help="The initial weights file from the pre-trained model "
                                       "(.npz in the reference's weight order)")
    p.add_argument("train_test_scenes_range", default="./restrepo_train_test_splits.json",
                   help="Path to the file containing the train-test splits")
    p.add_argument("--iterations", type=int, default=100000, help="Number of updates")
    p.add_argument("--validate_every", type=int, default=10)
    p.add_argument("--snapshot_every", type=int, default=100)
    p.add_argument("--batch_size", type=int, default=1000,
                   help="Number of rays used for a training step (default=1000)")
    p.add_argument("--repeat_from_neighboring_views", type=int, default=10)
    p.add_argument("--window", type=int, default=4,
                   help="Number of neighboring views from which to select batches (default=4)")
    p.add_argument("--n_test_samples", type=int, default=1000,
                   help="Number of randomly sampled rays used for testing")
    p.add_argument("--initial_gamma", type=float, default=0.031)
    p.add_argument("--gamma_range", type=ta._floats, default="1e-3,0.99",
                   help="The allowed values of gamma during training (default=(1e-3, 0.99))")
    p.add_argument("--train_with_gamma", action="store_true", help="Also learn the gamma prior")
    p.add_argument("--batch_norm", choices=["frozen", "batch"], default="frozen",
                   help="frozen: the CNN runs with its moving statistics while its weights train "
                        "(the reference's graph); batch: batch statistics in the steps")
    p.add_argument("--seed", type=int, default=0, help="Seed for the PRNG")
    ta.add_nn_arguments(p)
    ta.add_generation_arguments(p)
    ta.add_dataset_related_arguments(p)
    ta.add_run_arguments(p)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.network_architecture not in ["simple_cnn"]:          # (as the reference, :158)
        raise ValueError("Expected argument %r but received %r"
                         % (["simple_cnn"], args.network_architecture))
    if args.sampling_policy != "sample_in_bbox":
        raise NotImplementedError(
            "--sampling_policy %s: end-to-end training marches the voxels of the bounding-box "
            "segment and maps evenly spaced planes on it to them, so it samples in the bounding "
            "box only; pretrain_network takes the other policies" % args.sampling_policy)
    from raynet_amd.scripts.forward_pass import load_model
    from raynet_amd.train_network.ray_sampler import RayBatchSampler, SceneBank
    from raynet_amd.train_network.trainer import Trainer, draw_validation_set
    ta.seed_everything(args.seed)
    output_directory = os.path.join(args.output_directory, experiment_tag(args))
    os.makedirs(output_directory, exist_ok=True)
    gp = ta.generation_parameters(args)
    training_dataset, testing_dataset = ta.datasets(args, args.testing_directory)
    train_scenes, test_scenes = ta.scenes_split(args.train_test_scenes_range)
    model = load_model(args.weight_file, "simple_cnn", in_channels=args.patch_shape[2])
    train_sampler = RayBatchSampler(SceneBank(training_dataset, gp), args.batch_size, mode="random",
                                    scenes_range=train_scenes, n_rays=args.n_test_samples,
                                    window=args.window, seed=args.seed)
    test_sampler = RayBatchSampler(
        SceneBank(testing_dataset, gp), min(args.batch_size, args.n_test_samples), mode="window",
        scenes_range=test_scenes, window=args.window, seed=args.seed + 1,
        n_rays=get_number_of_neighboring_rays_test_set(args.dataset_type, args.n_test_samples))
    validation = draw_validation_set(test_sampler, args.n_test_samples)
    trainer = Trainer(model, "raynet", args.neighbors + 1, output_directory, loss=args.loss,
                      optimizer=args.optimizer, lr=args.lr, momentum=args.momentum,
                      weight_decay=args.weight_decay, clipnorm=0.1, batch_norm=args.batch_norm,
                      gamma=args.initial_gamma, gamma_range=args.gamma_range,
                      train_with_gamma=args.train_with_gamma, bp_iterations=args.bp_iterations)
    trainer.fit(train_sampler, validation, args.iterations, args.validate_every,
                args.snapshot_every, resume=args.resume, log=print)
    return trainer


if __name__ == "__main__":
    main(sys.argv[1:])
