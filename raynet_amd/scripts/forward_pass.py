#!/usr/bin/env python3
"""The caller of the hot path: `raynet_forward` of the reference (raynet/scripts/forward_pass.py:29-146)
with the flags that reach the path -- same names, same defaults -- on MI355X.

    python -m raynet_amd.scripts.forward_pass DATASET_DIR OUT_DIR --dataset_type restrepo \\
        --forward_pass_factory raynet --depth_planes 32 --grid_shape 64,64,32 ...

Loads a scene (Restrepo or DTU layout), builds the MV-CNN twin (random weights unless
--weight_file is given: a `.npz` holding the reference's weight list in the reference's own
order, raynet/models.py:329-339 -- `numpy.savez(path, *model.get_weights())` on the Keras
side; HDF5 itself cannot be read in this image -- or a torch state_dict of the twin), runs `forward_pass(scene, (start, end, skip_every + 1))` and writes one `depth_%03d.npy`
((H, W) float32) per reference image, the wire format of scripts/forward_pass.py:136-142.
--depth_statistics (raynet factory, resident schedule) writes `confidence_%03d.npy`,
`expected_depth_%03d.npy` and `depth_std_%03d.npy` of the same shape next to each of them: what
the model's depth distribution says about the pixel (forward_pass.DepthStatistics).
--save_occupancy (raynet factory) writes `occupancy.npz`: the occupancy probability of every voxel
after the pass, with the bounding box and the grid shape (volume.OccupancyVolume).
"""
import argparse
import os
import sys

import numpy as np

from . import scene_flags


def _floats(x):
    return tuple(map(float, x.split(",")))


def build_parser():
    p = argparse.ArgumentParser(description=("Do a forward pass and estimate the per pixel depth "
                                             "for the images of a scene"))
    p.add_argument("dataset_directory", help="Directory containing the input data")
    p.add_argument("output_directory", help="Directory to save the output data")
    p.add_argument("--weight_file", help="MV-CNN weights: .npz in the reference's weight order "
                                         "(models.py:329-339) or a torch state_dict of the twin")
    p.add_argument("--schedule", choices=["resident", "reference"], default="resident",
                   help="raynet factory: per-ray columns resident in HBM (grouped by the free "
                        "memory) / the reference's literal recompute-everything schedule")
    p.add_argument("--filter_out", action="store_true", help="Filter out rays with zero ground-truth")
    # scripts/arguments.py:146-223 (generation)
    p.add_argument("--patch_shape", type=scene_flags.ints, default="11,11,3")
    p.add_argument("--padding", default=None, type=int)
    p.add_argument("--depth_planes", type=int, default=32)
    p.add_argument("--neighbors", type=int, default=4)
    p.add_argument("--grid_shape", type=scene_flags.ints, default="256,256,128")
    p.add_argument("--maximum_number_of_marched_voxels", type=int, default=650)
    p.add_argument("--sampling_policy",
                   choices=["sample_in_bbox", "sample_in_range", "sample_in_disparity"],
                   default="sample_in_bbox",
                   help="Where on the viewing ray the depth planes lie (multi_view_cnn factory; "
                        "the voxel-space factories sample in the bounding box only)")
    p.add_argument("--depth_range", type=_floats, default="3.0,7.0",
                   help="The depth range used when sampling planes in range")
    # :302-329 (dataset) and :347-358 (indexing)
    scene_flags.add_arguments(p)
    p.add_argument("--neighbors_by_overlap", action="store_true",
                   help="A frame's neighbours are the frames that share the most of the scene's "
                        "bounding box with it at a useful triangulation angle (at most 64 images; "
                        "raynet_amd.view_selection), not file order or camera distance")
    # :335-345 (mrf)
    p.add_argument("--initial_gamma_prior", type=float, default=0.05)
    p.add_argument("--bp_iterations", type=int, default=3)
    # :362-379 (forward pass factory)
    p.add_argument("--forward_pass_factory",
                   choices=["multi_view_cnn", "multi_view_cnn_voxel_space", "raynet"],
                   default="raynet")
    p.add_argument("--rays_batch", type=int, default=130000)
    p.add_argument("--network_architecture", choices=["simple_cnn"], default="simple_cnn")
    p.add_argument("--depth_statistics", action="store_true",
                   help="raynet factory: also write confidence_%%03d.npy, expected_depth_%%03d.npy "
                        "and depth_std_%%03d.npy per reference image")
    p.add_argument("--save_occupancy", action="store_true",
                   help="raynet factory: also write occupancy.npz, the occupancy probability of "
                        "every voxel after the pass (raynet_amd.volume.OccupancyVolume; "
                        "raynet_amd.scripts.render_volume reads it)")
    return p


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def load_model(weight_file=None, architecture="simple_cnn", in_channels=3, device="cuda"):
    """The MV-CNN twin with the weights of `weight_file` (see --weight_file)."""
    import torch
    from raynet_amd.models import get_nn
    model = get_nn(architecture)(in_channels=in_channels).to(device)
    if weight_file:
        if str(weight_file).endswith(".npz"):
            model.load_reference_weights(weight_file)
        else:
            model.load_state_dict(torch.load(weight_file, map_location=device))
    return model


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.depth_statistics and (args.forward_pass_factory != "raynet" or
                                  args.schedule != "resident"):
        parser.error("--depth_statistics needs --forward_pass_factory raynet --schedule resident")
    if args.save_occupancy and args.forward_pass_factory != "raynet":
        parser.error("--save_occupancy needs --forward_pass_factory raynet: only the MRF keeps an "
                     "occupancy per voxel (%s estimates depth per ray)" % args.forward_pass_factory)
    if args.sampling_policy != "sample_in_bbox" and args.forward_pass_factory != "multi_view_cnn":
        parser.error("--sampling_policy %s needs --forward_pass_factory multi_view_cnn: the "
                     "voxel-space factories (%s) march the voxels of the bounding-box segment"
                     % (args.sampling_policy, args.forward_pass_factory))
    scene_flags.check(parser, args)
    if args.neighbors_by_overlap and args.select_neighbors_based_on != "filesystem":
        parser.error("--neighbors_by_overlap replaces --select_neighbors_based_on %s: give one of "
                     "them" % args.select_neighbors_based_on)
    import torch
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory

    if not os.path.exists(args.output_directory):
        os.makedirs(args.output_directory)
    if isinstance(args.patch_shape, str):
        args.patch_shape = scene_flags.ints(args.patch_shape)
    if isinstance(args.grid_shape, str):
        args.grid_shape = scene_flags.ints(args.grid_shape)
    if isinstance(args.depth_range, str):
        args.depth_range = _floats(args.depth_range)
    args.grid_shape = np.array(args.grid_shape, dtype=np.int32)
    generation_params = GenerationParameters.from_options(args)

    scene = scene_flags.open_scene(args)
    if args.neighbors_by_overlap:
        try:
            scene.use_overlap_neighbors()
        except ValueError as e:             # (more than 64 images)
            parser.error("--neighbors_by_overlap: %s" % e)
    model = load_model(args.weight_file, args.network_architecture,
                       in_channels=scene.get_image(0).image.shape[2])

    cls = get_forward_pass_factory(args.forward_pass_factory)
    kwargs = dict(filter_out_rays=args.filter_out)
    if args.forward_pass_factory == "raynet":
        kwargs["bp_iterations"] = args.bp_iterations
        kwargs["schedule"] = args.schedule
    fp = cls(model, generation_params, args.sampling_policy, scene.image_shape, args.rays_batch,
             **kwargs)

    # (the range goes to the driver as given, not clamped to the scene as scene_flags.frames
    # does: the driver walks it and the files are numbered by counting along)
    start, end = args.start_end
    ref_idx = start
    more = dict(with_statistics=True) if args.depth_statistics else {}
    for S in fp.forward_pass(scene, (start, end, args.skip_every + 1), **more):
        stats = None
        if args.depth_statistics:
            S, stats = S
        # (with a process group the rays are sharded and image k's map is assembled by ONE rank,
        # forward_pass.map_owner: the other ranks get None for it and leave its file alone)
        if S is not None:
            np.save(os.path.join(args.output_directory, "depth_%03d.npy" % (ref_idx,)), S)
        if stats is not None:
            for name in stats.FIELDS:
                np.save(os.path.join(args.output_directory, "%s_%03d.npy" % (name, ref_idx)),
                        getattr(stats, name))
        ref_idx += args.skip_every + 1
    if args.save_occupancy and _rank() == 0:
        # (the accumulator is the same on every rank after the exchange: one rank writes)
        fp.occupancy_volume().save(os.path.join(args.output_directory, "occupancy.npz"))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
