"""The texture flags of the scripts that write or render a surface mesh (fuse_depth_maps,
render_volume --mesh, render_mesh): one statement of their names, their checks and the step they
ask for.  mesh_flags' stages change the surface; the texture is baked from
the finished one, after all of them."""
import os

TEXTURE_FLAGS = ("texture", "texture_mode", "texture_normals")
MIN_T, MAX_T = 1, 1024
MAX_FRAMES = 32


def add_arguments(p, nearest=False):
    p.add_argument("--texture", type=int, default=None, metavar="T",
                   help="Bake the frames' images into a texture atlas of T texel steps per chart "
                        "leg (%d..%d)" % (MIN_T, MAX_T))
    p.add_argument("--texture_mode", choices=["blend", "best"], default=None,
                   help="--texture: the weighted mean of the frames that see a texel (default), or "
                        "the best one")
    p.add_argument("--texture_normals", choices=["face", "vertex"], default=None,
                   help="--texture: test a texel against its face's normal (default) or the "
                        "interpolated vertex normals")
    if nearest:
        p.add_argument("--texture_nearest", action="store_true",
                       help="--texture: look the nearest texel up instead of the bilinear four")


def check(parser, args, mesh_requested=True):
    """parser.error for a T out of range, a sub-flag without --texture, or --texture without the
    mesh file it is written beside."""
    sub = [name for name in ("texture_mode", "texture_normals", "texture_nearest")
           if getattr(args, name, None)]
    if args.texture is None:
        if sub:
            parser.error("--%s goes with --texture T" % sub[0])
        return
    if not MIN_T <= args.texture <= MAX_T:
        parser.error("--texture takes the texel steps per chart leg, %d..%d, got %d"
                     % (MIN_T, MAX_T, args.texture))
    if not mesh_requested:
        parser.error("--texture goes with --mesh PATH: the atlas is written beside the mesh file")


def check_frames(parser, args, frames):
    if args.texture is not None and len(frames) > MAX_FRAMES:
        parser.error("--texture: %d frames, at most %d per mesh; choose them with --start_end / "
                     "--skip_every" % (len(frames), MAX_FRAMES))


def check_color_frames(parser, args, frames):
    """--color blends the frames per vertex under the same limit."""
    if args.color and len(frames) > MAX_FRAMES:
        parser.error("--color: %d frames, at most 32 per mesh; choose them with --start_end / "
                     "--skip_every" % len(frames))


def bake(parser, args, mesh, scene, frames, tol):
    """-> texture.MeshTexture of the finished mesh from the frames, with --color's tolerance."""
    if mesh.empty or not frames:
        parser.error("--texture: %s" % ("the surface is empty" if mesh.empty else
                                        "--start_end selects no frame of the scene"))
    try:
        return mesh.textured(scene, frames, args.texture, tol, mode=args.texture_mode or "blend",
                             normals=args.texture_normals or "face")
    except ValueError as e:             # (an atlas beyond the largest the library addresses)
        parser.error("--texture: %s" % e)


def write(parser, args, mesh, scene, frames, tol, mesh_path):
    """The OBJ triple beside `mesh_path`, with its stem -> the three paths."""
    baked = bake(parser, args, mesh, scene, frames, tol)
    return mesh.save_obj(os.path.splitext(mesh_path)[0] + ".obj", baked)
