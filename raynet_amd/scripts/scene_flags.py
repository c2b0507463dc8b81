"""The scene flags of the scripts that open a scene and walk some of its frames (forward_pass,
render_volume, render_mesh, fuse_depth_maps, filter_depth_maps, compute_metrics,
convert_to_pointcloud): one statement of their names, their checks, the scene they open, the frames
they choose and the per-frame maps they read (the reference's scripts/arguments.py:300-358).

--dataset_type restrepo|dtu        the layout of DATASET_DIR (default restrepo)
--scene_idx N                      dtu: the scan number
--illumination_condition C         dtu: which of a scan's lightings (default max)
--select_neighbors_based_on filesystem|distance
                                   a frame's neighbours by file order (default) or camera distance

The frames, in one of two forms:
--start_end START,END --skip_every K   frames START, START + K + 1, ... below END and below the
                                       scene's number of images (defaults 0,5 and 0)
--frame_idxs A:B:C | I,J,K | I         a slice or a list of the scene's frames (default ":", all):
                                       compute_metrics and convert_to_pointcloud, whose frames are
                                       "the ordered prediction files" of the reference
"""
import os

import numpy as np


def ints(x):
    return tuple(map(int, x.split(",")))


def frame_idxs_type(arg):
    """"a:b:c" -> slice, "1,2,5" -> list, "3" -> [3] (scripts/slicing.py:8-18)."""
    if ":" in arg:
        return slice(*[int(x) if x != "" else None for x in arg.split(":")])
    if "," in arg:
        return [int(x) for x in arg.split(",")]
    return [int(arg)]


def find_format(input_directory, key, idx):
    """convert_to_pointcloud.py:30-35: "<key>_%d.npy" if that file of frame idx exists, else
    "<key>_%03d.npy"."""
    if os.path.isfile(os.path.join(input_directory, "%s_%d.npy" % (key, idx))):
        return key + "_%d.npy"
    return key + "_%03d.npy"


def add_arguments(p, scene_idx=1, frames="start_end"):
    p.add_argument("--dataset_type", choices=["restrepo", "dtu"], default="restrepo")
    p.add_argument("--scene_idx", default=scene_idx, type=int, help="DTU: the scan number")
    p.add_argument("--select_neighbors_based_on", choices=["filesystem", "distance"],
                   default="filesystem")
    p.add_argument("--illumination_condition", default="max")
    if frames == "start_end":
        p.add_argument("--start_end", type=ints, default="0,5")
        p.add_argument("--skip_every", type=int, default=0)
    else:
        p.add_argument("--frame_idxs", type=frame_idxs_type, default=":",
                       help="Choose the frames that correspond to the ordered prediction files")


def check(parser, args):
    """Converts the frame flag's string default; parser.error for a --start_end that is no pair."""
    if hasattr(args, "frame_idxs"):
        if isinstance(args.frame_idxs, str):
            args.frame_idxs = frame_idxs_type(args.frame_idxs)
        return
    if isinstance(args.start_end, str):
        args.start_end = ints(args.start_end)
    if len(args.start_end) != 2:
        parser.error("--start_end takes two numbers, START,END")


def open_scene(args):
    from raynet_amd.common import scene
    if args.dataset_type == "dtu":
        return scene.get_scene("dtu", args.dataset_directory, args.scene_idx,
                               illumination=args.illumination_condition,
                               select_neighbors_based_on=args.select_neighbors_based_on)
    return scene.get_scene("restrepo", args.dataset_directory,
                           select_neighbors_based_on=args.select_neighbors_based_on)


def frames(parser, args, scene, required=True):
    """-> the indices of the chosen frames of the scene.  required: parser.error for a --start_end
    that selects none (--frame_idxs has no such error, and needs no parser)."""
    if hasattr(args, "frame_idxs"):
        return [int(i) for i in np.arange(scene.n_images)[args.frame_idxs]]
    start, end = args.start_end
    chosen = list(range(start, min(end, scene.n_images), args.skip_every + 1))
    if required and not chosen:
        parser.error("--start_end selects no frame of the scene")
    return chosen


def load_maps(parser, directory, key, frames):
    """-> the arrays of directory/<key>_%d.npy (or _%03d.npy, whichever the first frame has) of the
    frames, as saved; parser.error if any is missing."""
    fmt = find_format(directory, key, frames[0])
    files = [os.path.join(directory, fmt % (i,)) for i in frames]
    missing = [f for f in files if not os.path.isfile(f)]
    if missing:
        parser.error("%d of %d %s maps are missing (first: %s)"
                     % (len(missing), len(files), key, missing[0]))
    return [np.load(f) for f in files]
