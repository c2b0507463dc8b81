"""The flags that smooth a mesh before it is written, shared by fuse_depth_maps and render_volume
--mesh (raynet_amd.smoothing):

--smooth N                Taubin smoothing, N iterations (a step with lambda, then one with mu)
--smooth_lambda L         the factor of the first step, in (0, 1] (default 0.5)
--smooth_mu M             the factor of the second step, in [-1, 0] (default -0.53; 0: plain
                          Laplacian smoothing, which shrinks the surface)
--smooth_max_move X       no coordinate of a vertex ends farther than X sides of the grid's smallest
                          voxel from where it started (default 1; inf: no limit)
--smooth_free_boundary    let the vertices on the mesh's border move too (default: they are pinned)

The smoothing runs on the cleaned mesh after the component filter, before normals, colours and
--mesh_cloud, and prints `smooth: N iterations, V vertices, farthest move M voxel sides`.
"""
import math

import numpy as np

FLAGS = ("smooth", "smooth_lambda", "smooth_mu", "smooth_max_move", "smooth_free_boundary")
MAX_ITERATIONS = 10000


def add_arguments(p):
    p.add_argument("--smooth", type=int, default=None,
                   help="Taubin smoothing of the mesh: this many iterations")
    p.add_argument("--smooth_lambda", type=float, default=None,
                   help="--smooth: the factor of the first step of an iteration, in (0, 1] (0.5)")
    p.add_argument("--smooth_mu", type=float, default=None,
                   help="--smooth: the factor of the second step, in [-1, 0] (-0.53; 0: none)")
    p.add_argument("--smooth_max_move", type=float, default=None,
                   help="--smooth: the farthest a coordinate may move, in sides of the grid's "
                        "smallest voxel (1; inf: no limit)")
    p.add_argument("--smooth_free_boundary", action="store_true", default=None,
                   help="--smooth: do not pin the vertices on the border of the mesh")


def given(args):
    return [f for f in FLAGS if getattr(args, f) is not None]


def check(parser, args):
    """parser.error (exit code 2, the flag's name in the message) for a value out of range, and
    for a flag of the smoothing without --smooth."""
    if args.smooth is not None and not 1 <= args.smooth <= MAX_ITERATIONS:
        parser.error("--smooth takes a number of iterations, 1..%d" % MAX_ITERATIONS)
    x = args.smooth_lambda
    if x is not None and not (math.isfinite(x) and 0.0 < x <= 1.0):
        parser.error("--smooth_lambda takes a factor in (0, 1]")
    x = args.smooth_mu
    if x is not None and not (math.isfinite(x) and -1.0 <= x <= 0.0):
        parser.error("--smooth_mu takes a factor in [-1, 0]")
    x = args.smooth_max_move
    if x is not None and not x > 0.0:
        parser.error("--smooth_max_move takes a positive number of voxel sides, or inf")
    if args.smooth is None and given(args):
        parser.error("--%s goes with --smooth N" % given(args)[0])


def apply(mesh, args, voxel):
    """The mesh smoothed by the flags given; the mesh itself without --smooth.  voxel: the three
    sides of a voxel of the grid, in scene units.  Prints the tally."""
    if args.smooth is None:
        return mesh
    side = float(np.min(np.asarray(voxel, np.float64)))
    limit = 1.0 if args.smooth_max_move is None else float(args.smooth_max_move)
    out = mesh.smoothed(iterations=args.smooth,
                        lam=0.5 if args.smooth_lambda is None else args.smooth_lambda,
                        mu=-0.53 if args.smooth_mu is None else args.smooth_mu,
                        fixed=None if args.smooth_free_boundary else "boundary",
                        max_move=limit * side)
    moved = np.abs(out.vertices.astype(np.float64) - mesh.vertices.astype(np.float64))
    moved = moved[np.isfinite(moved)]
    print("smooth: %d iterations, %d vertices, farthest move %.3f voxel sides"
          % (args.smooth, len(out.vertices), float(moved.max()) / side if moved.size else 0.0))
    return out
