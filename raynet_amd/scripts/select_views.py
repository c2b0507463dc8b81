#!/usr/bin/env python3
"""Which frames of a scene belong together, and which cover a surface.

    python -m raynet_amd.scripts.select_views DATASET_DIR OUT.json --dataset_type dtu \\
        --scene_idx 24 --neighbors 4 [--mesh MESH.ply --cover 32]

Takes the frames of --start_end / --skip_every (at most 64), asks every one of them which centres of
a coarse grid over the scene's bounding box it sees, and writes to OUT.json
  frames      the frame indices, in the order of the matrix' rows
  pairs       the symmetric matrix: on the diagonal the grid centres every frame sees, elsewhere
              the centres two frames share at a triangulation angle within --min_angle .. --max_angle
  neighbors   per frame its --neighbors best neighbours (frame indices), the best first
and with --mesh MESH.ply also
  cover       the frames in the order a greedy covering set of the mesh's vertices takes them (at
              most --cover of them), `gains`, the vertices each added, and `short`, the number of
              vertices fewer than --view_redundancy of the chosen frames see.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import scene_flags

MAX_FRAMES = 64


def build_parser():
    p = argparse.ArgumentParser(description="Choose views: pair overlaps, neighbours, covering sets")
    p.add_argument("dataset_directory", help="Directory containing the input data")
    p.add_argument("output_file", help="The JSON file to write")
    p.add_argument("--neighbors", type=int, default=4, help="Neighbours listed per frame")
    p.add_argument("--proxy_grid", type=scene_flags.ints, default="32,32,32",
                   help="The grid over the bounding box whose centres stand in for the scene")
    p.add_argument("--min_angle", type=float, default=2.0,
                   help="The smallest triangulation angle that counts, in degrees")
    p.add_argument("--max_angle", type=float, default=45.0,
                   help="The largest triangulation angle that counts, in degrees")
    p.add_argument("--mesh", default=None, help="Also write the covering order for this mesh (PLY)")
    p.add_argument("--cover", type=int, default=32, help="--mesh: frames to choose at the most")
    p.add_argument("--view_redundancy", type=int, default=1,
                   help="--mesh: a vertex is covered once this many chosen frames see it")
    p.add_argument("--depth_tolerance", type=float, default=None,
                   help="--mesh: the slack of the occlusion test in scene units (default: the "
                        "diagonal of a --proxy_grid cell)")
    scene_flags.add_arguments(p)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    if isinstance(args.proxy_grid, str):
        args.proxy_grid = scene_flags.ints(args.proxy_grid)
    if len(args.proxy_grid) != 3 or min(args.proxy_grid) < 1:
        parser.error("--proxy_grid takes three positive sizes, GX,GY,GZ")
    if not 0.0 <= args.min_angle <= args.max_angle <= 90.0:
        parser.error("--min_angle / --max_angle take degrees with 0 <= min <= max <= 90")
    if args.neighbors < 0:
        parser.error("--neighbors takes a number that is 0 or more")
    if not 1 <= args.view_redundancy <= MAX_FRAMES:
        parser.error("--view_redundancy takes 1..%d" % MAX_FRAMES)
    if args.cover < 1:
        parser.error("--cover takes a positive number of frames")
    if args.depth_tolerance is not None and not 0.0 <= args.depth_tolerance < float("inf"):
        parser.error("--depth_tolerance takes a finite distance, 0 or more")
    if args.mesh is not None and not os.path.isfile(args.mesh):
        parser.error("%s: no such file" % args.mesh)
    from raynet_amd.common.scene import get_voxel_grid
    from raynet_amd.view_selection import view_overlap

    scene = scene_flags.open_scene(args)
    frames = scene_flags.frames(parser, args, scene)
    if len(frames) > MAX_FRAMES:
        parser.error("%d frames, at most %d per call; thin them with --start_end / --skip_every"
                     % (len(frames), MAX_FRAMES))
    cameras = [scene.get_image(i).camera for i in frames]
    centres = get_voxel_grid(scene.bbox, args.proxy_grid).reshape(3, -1).T
    overlap = view_overlap(centres, cameras, scene.image_shape, min_angle=args.min_angle,
                           max_angle=args.max_angle)
    k = min(args.neighbors, len(frames) - 1)
    out = dict(frames=frames, pairs=overlap.pairs.tolist(),
               neighbors={str(f): [frames[j] for j in overlap.neighbors(r, k)]
                          for r, f in enumerate(frames)})
    if args.mesh is not None:
        from raynet_amd.volume import SurfaceMesh
        mesh = SurfaceMesh.load_ply(args.mesh)
        if mesh.empty:
            parser.error("%s: the mesh is empty, there is no surface to cover" % args.mesh)
        tol = args.depth_tolerance
        if tol is None:
            box = np.asarray(scene.bbox, np.float64).reshape(6)
            tol = float(np.sqrt((((box[3:] - box[:3]) / np.asarray(args.proxy_grid)) ** 2).sum()))
        chosen, gains, short = mesh.best_frames(scene, frames, args.cover, tol,
                                                redundancy=args.view_redundancy, return_stats=True)
        out["cover"] = dict(frames=chosen, gains=gains, short=short, vertices=len(mesh.vertices),
                            redundancy=args.view_redundancy, tolerance=tol)
        print("cover: frames %s; %d of %d vertices still short"
              % (",".join(str(i) for i in chosen), short, len(mesh.vertices)))
    with open(args.output_file, "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
