"""The flags that simplify a mesh before it is written, shared by fuse_depth_maps and render_volume
--mesh (raynet_amd.simplify):

--simplify X                 vertex clustering: the vertices that share a cell of X voxel sides of
                             the grid per axis (a positive, finite number) become one vertex at
                             their mean; the cells are anchored at the grid's bounding-box minimum
--simplify_keep_duplicates   keep the duplicate faces a collapsed thin sheet leaves (default: of
                             the faces that name the same three vertices the first one stays)

The simplification runs on the cleaned mesh after the component filter, before --smooth, normals,
colours and --mesh_cloud, and prints `simplify: cell X voxel sides, V -> V' vertices, F -> F' faces`.
"""
import math

import numpy as np

FLAGS = ("simplify", "simplify_keep_duplicates")


def add_arguments(p):
    p.add_argument("--simplify", type=float, default=None,
                   help="Vertex clustering of the mesh: cells of this many voxel sides per axis")
    p.add_argument("--simplify_keep_duplicates", action="store_true", default=None,
                   help="--simplify: keep the duplicate faces of collapsed thin sheets")


def given(args):
    return [f for f in FLAGS if getattr(args, f) is not None]


def check(parser, args):
    """parser.error (exit code 2, the flag's name in the message) for a value out of range, and
    for --simplify_keep_duplicates without --simplify."""
    x = args.simplify
    if x is not None and not (math.isfinite(x) and x > 0.0):
        parser.error("--simplify takes a positive, finite number of voxel sides")
    if args.simplify is None and given(args):
        parser.error("--%s goes with --simplify X" % given(args)[0])


def apply(mesh, args, voxel, origin):
    """The mesh simplified by the flags given; the mesh itself without --simplify.  voxel: the
    three sides of a voxel of the grid, origin: the minimum of its bounding box, in scene units.
    Prints the tally."""
    if args.simplify is None:
        return mesh
    cell = float(args.simplify) * np.asarray(voxel, np.float64)
    anchor = np.asarray(origin, np.float64)
    if len(mesh.vertices):
        # whole cells in front of the bounding box where the surface reaches out of it (the closing
        # faces of an occupancy volume lie one voxel outside): the anchor stays the box's minimum
        low = np.nanmin(np.where(np.isfinite(mesh.vertices), mesh.vertices, np.nan).astype(np.float64),
                        axis=0)
        steps = np.where(np.isfinite(low), np.floor((low - anchor) / cell), 0.0)
        anchor = anchor + np.minimum(steps, 0.0) * cell
    out = mesh.simplified(cell, origin=anchor,
                          drop_duplicate_faces=not args.simplify_keep_duplicates)
    print("simplify: cell %g voxel sides, %d -> %d vertices, %d -> %d faces"
          % (args.simplify, len(mesh.vertices), len(out.vertices), len(mesh.faces), len(out.faces)))
    return out
