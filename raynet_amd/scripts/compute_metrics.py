#!/usr/bin/env python3
"""Metrics of a 3D reconstruction (the reference's raynet/scripts/compute_metrics.py:56-177).

    python -m raynet_amd.scripts.compute_metrics DATASET_DIR PREDICTIONS_DIR METRIC [METRIC ...]

reads the predicted depth maps PREDICTIONS_DIR/depth_%03d.npy of the chosen frames (what
raynet_amd.scripts.forward_pass writes), turns them into the predicted point cloud, saves it
as OUTPUT_DIR/predicted_pc_s_%d.ply and prints `name mean: ... median: ...` per metric:

    ppmde                 per-pixel mean depth error against the ground-truth depth maps
    accuracy              predicted points -> nearest ground-truth point (the mesh's VERTICES)
    completeness          ground-truth points -> nearest predicted point
    surface_accuracy      predicted points -> nearest point of the ground-truth mesh's SURFACE
    surface_completeness  --surface_samples area-weighted samples of that surface (--seed)
                          -> nearest predicted point

DATASET_DIR is the scene's directory (Restrepo) or the DTU root with --scene_idx, as for
raynet_amd.scripts.forward_pass.  The flags are the reference's, with its defaults, but for
--min_distance: the VoxelMask / ReduceDensity filters live in raynet_amd.metrics, their factory
(`build_filter_factory`) and the --min_distance flag in raynet_amd.scripts.convert_to_pointcloud,
and `run(scene, args, filter_factory=...)` here hands a factory to every cloud metric; from
the command line the metrics run with an empty FiltersFactory.  The PLY coloured by a metric's
value is Pointcloud.save_colored_ply.
"""
import argparse
import os
import sys

import numpy as np

from . import scene_flags
from .scene_flags import frame_idxs_type      # (its home until the scripts shared their flags)

METRICS = ["ppmde", "accuracy", "completeness", "surface_accuracy", "surface_completeness"]


def build_parser():
    p = argparse.ArgumentParser(description="Compute the 3D reconstruction metrics")
    p.add_argument("dataset_directory", help="The dataset to load")
    p.add_argument("predictions_directory", help="The directory containing the model's predictions")
    p.add_argument("metric", nargs="+", choices=METRICS, help="Choose a metric")
    p.add_argument("--output_directory", default="/tmp/",
                   help="The directory to save the predicted point cloud")
    p.add_argument("--predicted_files_format", default="depth_%03d.npy",
                   help="The format for the predicted file")
    p.add_argument("--use_pc_from_depthmap", action="store_true",
                   help="Estimate the ground-truth point cloud from the depth images")
    # scripts/arguments.py:300-330 (dataset).  --scene_idx defaults to 0 here, the reference's
    # default for this script: the output file names carry it (predicted_pc_s_%d.ply)
    scene_flags.add_arguments(p, scene_idx=0, frames="frame_idxs")
    # :259-297 (metrics)
    p.add_argument("--borders", default=40, type=int,
                   help="The number of pixels to drop from the borders of the image")
    p.add_argument("--truncate", default=float("inf"), type=float,
                   help="Truncate all distances to this number if they are larger")
    p.add_argument("--consistency_threshold", default=0.75, type=float)
    p.add_argument("--n_neighbors", default=5, type=int,
                   help="Number of views considered during the consistency check")
    p.add_argument("--with_consistency_check", action="store_true")
    # the surface metrics
    p.add_argument("--surface_samples", default=1000000, type=int,
                   help="surface_completeness: area-weighted samples of the ground-truth surface")
    p.add_argument("--seed", default=0, type=int, help="surface_completeness: the samples' seed")
    return p


def build_metric(name, args, filter_factory=None):
    from raynet_amd.metrics import (Accuracy, Completeness, FiltersFactory,
                                    PerPixelMeanDepthError, SurfaceAccuracy,
                                    SurfaceCompleteness)
    filters = filter_factory if filter_factory is not None else FiltersFactory([])
    if name == "ppmde":
        return PerPixelMeanDepthError(args.borders)
    if name == "accuracy":
        return Accuracy(filters, args.truncate, args.borders, args.use_pc_from_depthmap)
    if name == "completeness":
        return Completeness(filters, args.truncate, args.borders, args.use_pc_from_depthmap)
    if name == "surface_accuracy":
        return SurfaceAccuracy(filters, args.truncate)
    if name == "surface_completeness":
        return SurfaceCompleteness(args.surface_samples, args.seed, filters, args.truncate)
    raise ValueError(name)


def main(argv=None):
    """-> {metric name: its values}, after printing each metric's mean and median."""
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    return run(scene_flags.open_scene(args), args)


def run(scene, args, filter_factory=None):
    """The script's body on a scene object (`args`: the parser's namespace).  filter_factory:
    a metrics.FiltersFactory for every cloud metric (None: no filters)."""
    from raynet_amd.pointcloud import get_pointcloud
    frame_idxs = scene_flags.frames(None, args, scene)
    depthmaps = [os.path.join(args.predictions_directory, args.predicted_files_format % (i,))
                 for i in frame_idxs]
    predicted_pointcloud = get_pointcloud(
        scene, frame_idxs, depthmaps, args.with_consistency_check, borders=args.borders,
        consistency_threshold=args.consistency_threshold, n_neighbors=args.n_neighbors)
    print("Saving predicted point-cloud for scene %d ..." % (args.scene_idx,))
    os.makedirs(args.output_directory, exist_ok=True)
    predicted_pointcloud.save_ply(
        os.path.join(args.output_directory, "predicted_pc_s_%d.ply" % (args.scene_idx,)))
    results = {}
    for name in args.metric:
        values, _ = build_metric(name, args, filter_factory).compute(
            scene, frame_idxs, depthmaps, predicted_pointcloud)
        results[name] = values
        print(name, " mean: ", values.mean(), " median: ", np.median(values))
    return results


if __name__ == "__main__":
    main(sys.argv[1:])
