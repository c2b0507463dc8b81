#!/usr/bin/env python3
"""Depth maps -> point cloud (the reference's raynet/scripts/convert_to_pointcloud.py:17-134).

    python -m raynet_amd.scripts.convert_to_pointcloud DATASET_DIR PREDICTIONS_DIR OUTPUT_DIR

reads the predicted depth maps PREDICTIONS_DIR/<pred_suffix>_%d.npy (or _%03d.npy, whichever
the first frame has) of the chosen frames, turns them into the predicted point cloud and saves
it as OUTPUT_DIR/predicted_pc_s_%d.ply.  With filters -- the scene's observation mask
(VoxelMask; DTU scans have one) and --min_distance d (ReduceDensity: no two kept points within
d; -1, the default, is off) -- the filtered cloud is saved as filtered_predicted_pc_s_%d.ply
as well, and each filter leaves its own PLY in OUTPUT_DIR.  The flags are the reference's, with
its defaults; --seed is new: the thinning's visiting order (the reference shuffles unseeded),
and so is --min_confidence X: pixels whose confidence (PREDICTIONS_DIR/confidence_%03d.npy, what
`forward_pass --depth_statistics` writes) is below X do not become points.  --color is new too: the
clouds are also saved with the colours of the chosen frames' images, as colored_predicted_pc_s_%d.ply
(and colored_filtered_predicted_pc_s_%d.ply when filters ran): a frame colours the points it sees,
with the predicted depth maps as occluders at the tolerance --consistency_threshold, and the frames
that see a point are blended (Pointcloud.colorize).  At most 32 frames.
--min_consistent_views K [--max_violations M --consistency_abs X --consistency_rel X] is new as well:
a pixel becomes a point only if at least K of the other chosen frames agree with its depth and at
most M see past it (raynet_amd.scripts.consistency_flags; at most 32 frames).
--with_consistency_check stays the reference's check; the two exclude each other.
"""
import argparse
import os
import sys

import numpy as np

from . import consistency_flags, scene_flags
from .scene_flags import find_format, frame_idxs_type     # (their home until the scripts shared them)


def build_filter_factory(scene, min_distance, output_directory=None, seed=0):
    """convert_to_pointcloud.py:17-27: [VoxelMask if the scene has an observation mask,
    ReduceDensity if min_distance != -1], in this order."""
    from raynet_amd.metrics import FiltersFactory, ReduceDensity, VoxelMask
    filters = []
    mask = scene.observation_mask
    if mask is not None:
        filters.append(VoxelMask(scene.bbox, mask, output_directory))
    if min_distance != -1:
        filters.append(ReduceDensity(min_distance, output_directory, seed=seed))
    return FiltersFactory(filters)


def build_parser():
    p = argparse.ArgumentParser(description="Transform the input depth maps to a pointcloud")
    p.add_argument("dataset_directory", help="The dataset to load")
    p.add_argument("predictions_directory", help="The directory containing the model's predictions")
    p.add_argument("output_directory", help="The directory to save the predicted point cloud")
    p.add_argument("--pred_suffix", default="depth",
                   help="The suffix for the predicted files (default=depth)")
    # scripts/arguments.py:300-330 (dataset).  --scene_idx defaults to 0 here, the reference's
    # default for this script: the output file names carry it (predicted_pc_s_%d.ply)
    scene_flags.add_arguments(p, scene_idx=0, frames="frame_idxs")
    # :259-297 (metrics)
    p.add_argument("--borders", default=40, type=int,
                   help="The number of pixels to drop from the borders of the image")
    p.add_argument("--truncate", default=float("inf"), type=float,
                   help="Truncate all distances to this number if they are larger")
    p.add_argument("--min_distance", default=-1, type=float,
                   help="Reduce the density of the points based on this distance")
    p.add_argument("--consistency_threshold", default=0.75, type=float)
    p.add_argument("--n_neighbors", default=5, type=int,
                   help="Number of views considered during the consistency check")
    p.add_argument("--with_consistency_check", action="store_true")
    p.add_argument("--seed", default=0, type=int,
                   help="--min_distance: the seed of the thinning's visiting order")
    p.add_argument("--min_confidence", default=None, type=float,
                   help="Drop the pixels whose confidence (confidence_%%03d.npy in the predictions "
                        "directory, from forward_pass --depth_statistics) is below this (default: off)")
    p.add_argument("--color", action="store_true",
                   help="Also write the clouds with the colours of the chosen frames' images "
                        "(colored_*.ply; the depth maps occlude, at --consistency_threshold)")
    consistency_flags.add_arguments(p)
    return p


def main(argv=None):
    """-> (predicted cloud, filtered cloud or None), after writing the PLY files."""
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    if args.color and not args.consistency_threshold >= 0:
        parser.error("--color: --consistency_threshold is the occlusion tolerance and cannot be "
                     "negative")
    consistency_flags.check(parser, args)
    if consistency_flags.requested(args) and args.with_consistency_check:
        parser.error("--min_consistent_views and --with_consistency_check (the reference's check) "
                     "exclude each other")
    return run(scene_flags.open_scene(args), args)


def run(scene, args):
    """The script's body on a scene object (`args`: the parser's namespace)."""
    from raynet_amd.pointcloud import get_pointcloud
    frame_idxs = scene_flags.frames(None, args, scene)
    os.makedirs(args.output_directory, exist_ok=True)
    filter_factory = build_filter_factory(scene, args.min_distance,
                                          output_directory=args.output_directory, seed=args.seed)
    fmt = find_format(args.predictions_directory, args.pred_suffix, frame_idxs[0])
    depthmaps = [os.path.join(args.predictions_directory, fmt % (i,)) for i in frame_idxs]
    confidence = {}
    if getattr(args, "min_confidence", None) is not None:
        # (not scene_flags.load_maps: no parser in reach here, get_pointcloud takes the paths,
        # and the message names the flag and the remedy)
        cfmt = find_format(args.predictions_directory, "confidence", frame_idxs[0])
        files = [os.path.join(args.predictions_directory, cfmt % (i,)) for i in frame_idxs]
        missing = [f for f in files if not os.path.isfile(f)]
        if missing:
            raise SystemExit(
                "--min_confidence: %d of %d confidence maps are missing (first: %s); write them "
                "with `forward_pass --depth_statistics`" % (len(missing), len(files), missing[0]))
        confidence = dict(confidences=files, min_confidence=args.min_confidence)
    if consistency_flags.requested(args):
        if len(frame_idxs) > consistency_flags.MAX_FRAMES:
            raise SystemExit("--min_consistent_views: %d frames, at most %d per run; choose them "
                             "with --frame_idxs" % (len(frame_idxs), consistency_flags.MAX_FRAMES))
        results = consistency_flags.run(args, scene, frame_idxs, [np.load(d) for d in depthmaps])
        confidence["keep_masks"] = [c.keep(args.min_consistent_views, args.max_violations)
                                    for c in results]
    predicted_pointcloud = get_pointcloud(
        scene, frame_idxs, depthmaps, args.with_consistency_check, borders=args.borders,
        consistency_threshold=args.consistency_threshold, n_neighbors=args.n_neighbors,
        **confidence)
    print("Saving predicted point-cloud for scene %d ..." % (args.scene_idx,))
    predicted_pointcloud.save_ply(
        os.path.join(args.output_directory, "predicted_pc_s_%d.ply" % (args.scene_idx,)))

    def save_colored(name):
        if getattr(args, "color", False):
            colors, _ = predicted_pointcloud.colorize(scene, frame_idxs, depthmaps,
                                                      tol=args.consistency_threshold)
            predicted_pointcloud.save_rgb_ply(
                os.path.join(args.output_directory, name % (args.scene_idx,)), colors)

    save_colored("colored_predicted_pc_s_%d.ply")
    unfiltered = predicted_pointcloud.points
    if not filter_factory.has_filters:
        return unfiltered, None
    predicted_pointcloud.filter(filter_factory)
    predicted_pointcloud.save_ply(
        os.path.join(args.output_directory, "filtered_predicted_pc_s_%d.ply" % (args.scene_idx,)))
    save_colored("colored_filtered_predicted_pc_s_%d.ply")
    return unfiltered, predicted_pointcloud.points


if __name__ == "__main__":
    main(sys.argv[1:])
