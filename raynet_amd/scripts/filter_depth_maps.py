#!/usr/bin/env python3
"""Check depth maps against each other and write the filtered maps.

    python -m raynet_amd.scripts.filter_depth_maps DATASET_DIR PREDICTIONS_DIR FILTERED_DIR \\
        --start_end 0,12 [--min_consistent_views 2 --max_violations 0 --consistency_rel 0.01]

PREDICTIONS_DIR holds `depth_%03d.npy` (--pred_suffix), one (H, W) map of distances to the camera
centre per frame of --start_end / --skip_every: what `raynet_amd.scripts.forward_pass` writes.
Every pixel of every map is put to the other chosen frames (raynet_amd.consistency, DESIGN.md
section 29): a frame agrees with a pixel whose point lies at the depth the frame recorded there,
within --consistency_abs + --consistency_rel * depth; it is violated where it sees past the point.
Per frame, FILTERED_DIR receives

    depth_%03d.npy    the map with 0 -- "no measurement" to fuse_depth_maps -- where fewer than
                      --min_consistent_views frames (default 2) agree or more than --max_violations
                      (default 0) are violated, float32
    agree_%03d.npy    how many frames agree with every pixel, uint8
    violate_%03d.npy  how many frames see past it, uint8

for fuse_depth_maps and convert_to_pointcloud (as their PREDICTIONS_DIR) and for inspection.  The
depth is read at the nearest pixel: the tolerance must exceed the depth step of one pixel of the
surfaces it is to confirm.  At most 32 frames per run.
"""
import argparse
import os
import sys

import numpy as np

from . import consistency_flags, scene_flags


def build_parser():
    p = argparse.ArgumentParser(description="Filter depth maps by cross-view consistency")
    p.add_argument("dataset_directory", help="Directory containing the input data")
    p.add_argument("predictions_directory", help="Directory of the depth maps (depth_%%03d.npy)")
    p.add_argument("output_directory", help="Directory to write the filtered maps and counts to")
    p.add_argument("--pred_suffix", default="depth",
                   help="The suffix for the predicted files (default=depth)")
    p.add_argument("--border", type=float, default=0.0,
                   help="Pixels to stay away from the edge of the depth maps")
    consistency_flags.add_arguments(p)
    scene_flags.add_arguments(p)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    if not 0.0 <= args.border < float("inf"):
        parser.error("--border takes a finite number of pixels, 0 or more")
    if args.min_consistent_views is None:
        args.min_consistent_views = 2               # the check is what this script is for
    consistency_flags.check(parser, args)
    scene = scene_flags.open_scene(args)
    frames = scene_flags.frames(parser, args, scene)
    consistency_flags.check_frames(parser, args, frames)
    depth_maps = [np.asarray(m, np.float32) for m in scene_flags.load_maps(
        parser, args.predictions_directory, args.pred_suffix, frames)]
    results = consistency_flags.run(args, scene, frames, depth_maps, args.border)
    os.makedirs(args.output_directory, exist_ok=True)
    for frame, c, depth in zip(frames, results, depth_maps):
        for name, array in (
                ("depth", c.filtered(depth, args.min_consistent_views, args.max_violations)),
                ("agree", c.agree_count), ("violate", c.violate_count)):
            np.save(os.path.join(args.output_directory, "%s_%03d.npy" % (name, frame)), array)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
