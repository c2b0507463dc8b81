"""The flags that drop floaters from a mesh before it is written, shared by fuse_depth_maps and
render_volume --mesh (raynet_amd.components):

--min_component_faces N      drop the connected components with fewer than N faces
--min_component_fraction X   drop those with fewer than X times the largest component's faces
--keep_largest K             keep only the K components with the most faces

Two vertices are connected if a face names both.  The filter runs on the cleaned mesh, before
normals, colours and --mesh_cloud, and prints `components: K found, k kept, F -> f faces`.
"""
import math

FLAGS = ("min_component_faces", "min_component_fraction", "keep_largest")


def add_arguments(p):
    p.add_argument("--min_component_faces", type=int, default=None,
                   help="Drop the connected components of the mesh with fewer faces than this")
    p.add_argument("--min_component_fraction", type=float, default=None,
                   help="Drop the components with fewer than this fraction of the largest one's faces")
    p.add_argument("--keep_largest", type=int, default=None,
                   help="Keep only this many components, the ones with the most faces")


def given(args):
    return [f for f in FLAGS if getattr(args, f) is not None]


def check(parser, args):
    """parser.error (exit code 2, the flag's name in the message) for a value out of range."""
    if args.min_component_faces is not None and args.min_component_faces < 1:
        parser.error("--min_component_faces takes a number of faces, 1 or more")
    if args.keep_largest is not None and args.keep_largest < 1:
        parser.error("--keep_largest takes a number of components, 1 or more")
    x = args.min_component_fraction
    if x is not None and not (math.isfinite(x) and 0.0 < x <= 1.0):
        parser.error("--min_component_fraction takes a fraction in (0, 1]")


def apply(mesh, args):
    """The mesh without its small components, by the flags given; the mesh itself if none is.
    Prints the tally."""
    if not given(args):
        return mesh
    from raynet_amd.components import filter_small
    out, found, kept = filter_small(mesh, args.min_component_faces, args.min_component_fraction,
                                    args.keep_largest)
    print("components: %d found, %d kept, %d -> %d faces"
          % (found, kept, len(mesh.faces), len(out.faces)))
    return out
