"""The flags that clean up a mesh before it is written, shared by fuse_depth_maps and render_volume
--mesh.  Four stages, in this order, each on the cleaned mesh and before normals, colours and
--mesh_cloud:

--min_component_faces N      drop the connected components with fewer than N faces
--min_component_fraction X   drop those with fewer than X times the largest component's faces
--keep_largest K             keep only the K components with the most faces
    Two vertices are connected if a face names both (raynet_amd.components).
    Prints `components: K found, k kept, F -> f faces`.

--fill_holes N               cap every simple boundary loop of 3..N edges (N in 3..65536) with a
                             vertex at the mean of its vertices and a fan of faces; longer loops
                             -- the outer rim of the surface -- and loops that are not simple stay
                             open.  After the component filter, so that the rim of a stray patch is
                             not capped into a pillow; before --simplify and --smooth, which then
                             treat the caps like the rest and find no rim to pin
    (raynet_amd.holes).  Prints
    `holes: K loops, k filled (s not simple, l longer than N), F -> F' faces`.

--simplify X                 vertex clustering: the vertices that share a cell of X voxel sides of
                             the grid per axis (a positive, finite number) become one vertex at
                             their mean; the cells are anchored at the grid's bounding-box minimum
--simplify_keep_duplicates   keep the duplicate faces a collapsed thin sheet leaves (default: of
                             the faces that name the same three vertices the first one stays)
    (raynet_amd.simplify).  Prints
    `simplify: cell X voxel sides, V -> V' vertices, F -> F' faces`.
--simplify_placement P       where the one vertex of a cell goes: `mean` (the default) or `quadric`,
                             the point nearest to the planes of the faces around the cell, which
                             keeps ridges, corners and eaves sharp where the mean rounds them off
--simplify_regularization X  --simplify_placement quadric: the pull back to the mean, as a share of
                             the faces' summed weights, in [2^-20, 1] (default 2^-10)
    (DESIGN.md section 28).  With `quadric` a second line:
    `placement: quadric, K of V' vertices moved, F fell back, farthest move M cell sides`.

--smooth N                   Taubin smoothing, N iterations (a step with lambda, then one with mu)
--smooth_lambda L            the factor of the first step, in (0, 1] (default 0.5)
--smooth_mu M                the factor of the second step, in [-1, 0] (default -0.53; 0: plain
                             Laplacian smoothing, which shrinks the surface)
--smooth_max_move X          no coordinate of a vertex ends farther than X sides of the grid's
                             smallest voxel from where it started (default 1; inf: no limit)
--smooth_free_boundary       let the vertices on the mesh's border move too (default: pinned)
    (raynet_amd.smoothing).  Prints
    `smooth: N iterations, V vertices, farthest move M voxel sides`.

--mesh_cloud PATH --mesh_samples N [--seed S]   also write N area-weighted points of the cleaned
                             surface as a point cloud (add_cloud_arguments / check_cloud)
"""
import math

import numpy as np

COMPONENT_FLAGS = ("min_component_faces", "min_component_fraction", "keep_largest")
SIMPLIFY_FLAGS = ("simplify", "simplify_keep_duplicates")
SMOOTH_FLAGS = ("smooth", "smooth_lambda", "smooth_mu", "smooth_max_move", "smooth_free_boundary")
FLAGS = COMPONENT_FLAGS + SIMPLIFY_FLAGS + SMOOTH_FLAGS
HOLE_FLAGS = ("fill_holes",)        # registered behind FLAGS; its stage runs after the components'
PLACEMENT_FLAGS = ("simplify_placement", "simplify_regularization")     # behind those; --simplify's
PLACEMENTS = ("mean", "quadric")
MIN_REGULARIZATION = 2.0 ** -20
MAX_ITERATIONS = 10000
MIN_HOLE_EDGES, MAX_HOLE_EDGES = 3, 65536


def add_arguments(p):
    p.add_argument("--min_component_faces", type=int, default=None,
                   help="Drop the connected components of the mesh with fewer faces than this")
    p.add_argument("--min_component_fraction", type=float, default=None,
                   help="Drop the components with fewer than this fraction of the largest one's faces")
    p.add_argument("--keep_largest", type=int, default=None,
                   help="Keep only this many components, the ones with the most faces")
    p.add_argument("--simplify", type=float, default=None,
                   help="Vertex clustering of the mesh: cells of this many voxel sides per axis")
    p.add_argument("--simplify_keep_duplicates", action="store_true", default=None,
                   help="--simplify: keep the duplicate faces of collapsed thin sheets")
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
    p.add_argument("--fill_holes", type=int, default=None,
                   help="Cap the boundary loops of the mesh that have at most this many edges")
    p.add_argument("--simplify_placement", choices=PLACEMENTS, default=None,
                   help="--simplify: the vertex of a cell at the mean of its members (mean) or "
                        "nearest to the planes of the faces around it (quadric)")
    p.add_argument("--simplify_regularization", type=float, default=None,
                   help="--simplify_placement quadric: the pull back to the mean, in [2^-20, 1] "
                        "(2^-10)")


def add_cloud_arguments(p):
    p.add_argument("--mesh_cloud", default=None,
                   help="Also write --mesh_samples points of the surface as a point cloud (PLY) here")
    p.add_argument("--mesh_samples", type=int, default=None,
                   help="--mesh_cloud: how many area-weighted points to draw")
    p.add_argument("--seed", type=int, default=0, help="--mesh_cloud: the seed of the samples")


def check_cloud(parser, args):
    if args.mesh_cloud and args.mesh_samples is None:
        parser.error("--mesh_cloud needs --mesh_samples N")
    if args.mesh_samples is not None and (not args.mesh_cloud or args.mesh_samples < 1):
        parser.error("--mesh_samples takes a positive number and goes with --mesh_cloud PATH")


def given(args, flags=FLAGS):
    return [f for f in flags if getattr(args, f, None) is not None]


def check(parser, args, mesh_requested=True):
    """parser.error (exit code 2, the flag's name in the message) for a value out of range, for a
    flag of a stage without the stage's own, and -- mesh_requested False: the script writes no
    mesh -- for any flag at all.  Stage by stage, in the order the stages run."""
    def needs_mesh(flags, what):
        if not mesh_requested and given(args, flags):
            parser.error("--%s goes with --mesh PATH: the %s the mesh's" % (given(args, flags)[0], what))

    if args.min_component_faces is not None and args.min_component_faces < 1:
        parser.error("--min_component_faces takes a number of faces, 1 or more")
    if args.keep_largest is not None and args.keep_largest < 1:
        parser.error("--keep_largest takes a number of components, 1 or more")
    x = args.min_component_fraction
    if x is not None and not (math.isfinite(x) and 0.0 < x <= 1.0):
        parser.error("--min_component_fraction takes a fraction in (0, 1]")
    needs_mesh(COMPONENT_FLAGS, "components are")

    n = getattr(args, "fill_holes", None)
    if n is not None and not MIN_HOLE_EDGES <= n <= MAX_HOLE_EDGES:
        parser.error("--fill_holes takes a number of edges, %d..%d" % (MIN_HOLE_EDGES, MAX_HOLE_EDGES))
    if not mesh_requested and n is not None:
        parser.error("--fill_holes goes with --mesh PATH: the holes are the mesh's")

    x = args.simplify
    if x is not None and not (math.isfinite(x) and x > 0.0):
        parser.error("--simplify takes a positive, finite number of voxel sides")
    if args.simplify is None and given(args, SIMPLIFY_FLAGS):
        parser.error("--%s goes with --simplify X" % given(args, SIMPLIFY_FLAGS)[0])
    needs_mesh(SIMPLIFY_FLAGS, "simplification is")

    x = getattr(args, "simplify_regularization", None)
    if x is not None and not MIN_REGULARIZATION <= x <= 1.0:
        parser.error("--simplify_regularization takes a share in [2^-20, 1]")
    if x is not None and getattr(args, "simplify_placement", None) != "quadric":
        parser.error("--simplify_regularization goes with --simplify_placement quadric")
    if args.simplify is None and given(args, PLACEMENT_FLAGS):
        parser.error("--%s goes with --simplify X" % given(args, PLACEMENT_FLAGS)[0])
    needs_mesh(PLACEMENT_FLAGS, "placement is")

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
    if args.smooth is None and given(args, SMOOTH_FLAGS):
        parser.error("--%s goes with --smooth N" % given(args, SMOOTH_FLAGS)[0])
    needs_mesh(SMOOTH_FLAGS, "smoothing is")


def voxel_sides(volume):
    """The three sides of a voxel of the volume's grid, in scene units (float64)."""
    bbox = volume.bbox.astype(np.float64)
    return (bbox[3:] - bbox[:3]) / np.array(volume.grid_shape, np.float64)


def voxel_diagonal(volume):
    """The diagonal of a voxel of the volume's grid, in scene units: the slack of the occlusion
    tests of --color and --texture."""
    return float(np.sqrt((voxel_sides(volume) ** 2).sum()))


def drop_components(mesh, args):
    """The mesh without its small components, by the flags given; the mesh itself if none is.
    Prints the tally."""
    if not given(args, COMPONENT_FLAGS):
        return mesh
    from raynet_amd.components import filter_small
    out, found, kept = filter_small(mesh, args.min_component_faces, args.min_component_fraction,
                                    args.keep_largest)
    print("components: %d found, %d kept, %d -> %d faces"
          % (found, kept, len(mesh.faces), len(out.faces)))
    return out


def fill_holes(mesh, args):
    """The mesh with its small holes capped; the mesh itself without --fill_holes (and for a
    namespace that does not know the flag).  Prints the tally."""
    n = getattr(args, "fill_holes", None)
    if n is None:
        return mesh
    out, stats = mesh.filled(n, return_stats=True)
    print("holes: %d loops, %d filled (%d not simple, %d longer than %d), %d -> %d faces"
          % (stats["loops"], stats["filled"], stats["not_simple"],
             stats["loops"] - stats["filled"] - stats["not_simple"], n, len(mesh.faces),
             len(out.faces)))
    return out


def simplify(mesh, args, voxel, origin):
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
    if getattr(args, "simplify_placement", None) != "quadric":
        out = mesh.simplified(cell, origin=anchor,
                              drop_duplicate_faces=not args.simplify_keep_duplicates)
        stats = None
    else:
        x = getattr(args, "simplify_regularization", None)
        out, stats = mesh.simplified(cell, origin=anchor,
                                     drop_duplicate_faces=not args.simplify_keep_duplicates,
                                     placement="quadric",
                                     regularization=2.0 ** -10 if x is None else x,
                                     return_stats=True)
    print("simplify: cell %g voxel sides, %d -> %d vertices, %d -> %d faces"
          % (args.simplify, len(mesh.vertices), len(out.vertices), len(mesh.faces), len(out.faces)))
    if stats is not None:
        print("placement: quadric, %d of %d vertices moved, %d fell back, farthest move %.3f cell "
              "sides" % (stats["moved"], len(out.vertices), stats["fell_back"],
                         stats["farthest_move"]))
    return out


def smooth(mesh, args, voxel):
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


def apply(mesh, args, volume):
    """The mesh of `volume` (its bbox and grid_shape give the voxel) through the stages whose flags
    are given: components, then fill_holes, then simplify, then smooth.  The mesh itself if no
    flag is."""
    voxel = voxel_sides(volume)
    mesh = drop_components(mesh, args)
    mesh = fill_holes(mesh, args)
    mesh = simplify(mesh, args, voxel, volume.bbox.astype(np.float64)[:3])
    return smooth(mesh, args, voxel)
