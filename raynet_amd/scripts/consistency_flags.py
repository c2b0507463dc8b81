"""The cross-view check flags of the scripts that consume depth maps (fuse_depth_maps,
convert_to_pointcloud, filter_depth_maps): one statement of their names, their checks and the step
they ask for (raynet_amd.consistency).  Without --min_consistent_views
nothing is checked and every output is what it was.

--min_consistent_views K  a pixel stays only if at least K of the other chosen frames agree with
                          its depth
--max_violations M        ... and at most M of them see past it (default 0)
--consistency_abs X       a frame agrees within X scene units (default 0) ...
--consistency_rel X       ... plus X times the depth it recorded (default 0.01)

The depth is read at the nearest pixel: the tolerance must exceed the depth step of one pixel of
the surfaces it is to confirm.  At most 32 frames per run.
"""
import numpy as np

SUB_FLAGS = ("max_violations", "consistency_abs", "consistency_rel")
MAX_FRAMES = 32
DEFAULT_REL = 0.01


def add_arguments(p):
    p.add_argument("--min_consistent_views", type=int, default=None, metavar="K",
                   help="Cross-view check: keep a pixel only if at least K other frames agree with it")
    p.add_argument("--max_violations", type=int, default=None, metavar="M",
                   help="--min_consistent_views: ... and at most M frames see past it (default 0)")
    p.add_argument("--consistency_abs", type=float, default=None, metavar="X",
                   help="--min_consistent_views: the absolute tolerance, scene units (default 0)")
    p.add_argument("--consistency_rel", type=float, default=None, metavar="X",
                   help="--min_consistent_views: the tolerance relative to the depth (default %g)"
                        % DEFAULT_REL)


def requested(args):
    return getattr(args, "min_consistent_views", None) is not None


def fill_defaults(args):
    for name, value in (("max_violations", 0), ("consistency_abs", 0.0),
                        ("consistency_rel", DEFAULT_REL)):
        if getattr(args, name, None) is None:
            setattr(args, name, value)


def check(parser, args):
    """parser.error for a sub-flag without --min_consistent_views or a value out of range; fills
    the defaults in where the check is asked for."""
    sub = [name for name in SUB_FLAGS if getattr(args, name, None) is not None]
    if not requested(args):
        if sub:
            parser.error("--%s goes with --min_consistent_views K" % sub[0])
        return
    fill_defaults(args)
    if args.min_consistent_views < 0:
        parser.error("--min_consistent_views takes a number of frames, 0 or more")
    if args.max_violations < 0:
        parser.error("--max_violations takes a number of frames, 0 or more")
    for name in ("consistency_abs", "consistency_rel"):
        if not 0.0 <= getattr(args, name) < float("inf"):
            parser.error("--%s takes a finite tolerance, 0 or more" % name)


def check_frames(parser, args, frames):
    if requested(args) and len(frames) > MAX_FRAMES:
        parser.error("--min_consistent_views: %d frames, at most %d per run; choose them with the "
                     "frame flags" % (len(frames), MAX_FRAMES))


def run(args, scene, frames, depth_maps, border=0.0, report=print):
    """-> the DepthConsistency of every frame's map, after a line per frame: how many measured
    pixels are dropped, as violated (more than --max_violations frames see past them) or as
    disagreeing (too few frames agree)."""
    from raynet_amd.consistency import check_depth_maps
    fill_defaults(args)
    results = check_depth_maps(depth_maps, scene=scene, frame_idxs=frames,
                               tol_abs=args.consistency_abs, tol_rel=args.consistency_rel,
                               border=border)
    for frame, c in zip(frames, results):
        violating = c.measured & (c.violate_count > args.max_violations)
        disagreeing = c.measured & ~violating & (c.agree_count < args.min_consistent_views)
        report("frame %d: %d of %d measured pixels dropped, %d disagreeing and %d violating"
               % (frame, int(violating.sum()) + int(disagreeing.sum()), int(c.measured.sum()),
                  int(disagreeing.sum()), int(violating.sum())))
    return results


def filter_maps(args, scene, frames, depth_maps, border=0.0, report=print):
    """-> the maps with 0 where a pixel is not kept ("no measurement" to the fusion)."""
    results = run(args, scene, frames, depth_maps, border, report)
    return [c.filtered(np.asarray(m, np.float32), args.min_consistent_views, args.max_violations)
            for c, m in zip(results, depth_maps)]
