"""The view-selection flags of the scripts that colour or texture a surface mesh (fuse_depth_maps,
render_volume --mesh, render_mesh): one statement of their names, their checks and the step they
ask for.

--select_views K        of the frames of --start_end / --skip_every (the candidates, at most 64)
                        give --color / --texture only the K <= 32 that between them see the most
                        of the finished mesh: a greedy covering set over its vertices, with the
                        tolerance the colour step is given
--view_redundancy R     --select_views: a vertex counts as covered once R chosen frames see it
                        (default 1)

Without --select_views nothing changes: the colour and texture steps get every frame.
"""
MAX_CANDIDATES = 64
MAX_CHOSEN = 32


def add_arguments(p):
    p.add_argument("--select_views", type=int, default=None, metavar="K",
                   help="--color / --texture: use only the K (1..%d) frames that between them see "
                        "the most of the mesh, of at most %d candidates"
                        % (MAX_CHOSEN, MAX_CANDIDATES))
    p.add_argument("--view_redundancy", type=int, default=None, metavar="R",
                   help="--select_views: a vertex is covered once R chosen frames see it (default 1)")


def requested(args):
    return args.select_views is not None


def check(parser, args, used=True):
    """parser.error for a K or R out of range, --view_redundancy without --select_views, or
    --select_views without a step that takes colours from the frames (`used`)."""
    if args.select_views is None:
        if args.view_redundancy is not None:
            parser.error("--view_redundancy goes with --select_views K")
        return
    if not 1 <= args.select_views <= MAX_CHOSEN:
        parser.error("--select_views takes the number of frames to keep, 1..%d, got %d"
                     % (MAX_CHOSEN, args.select_views))
    if args.view_redundancy is not None and not 1 <= args.view_redundancy <= MAX_CANDIDATES:
        parser.error("--view_redundancy takes 1..%d, got %d" % (MAX_CANDIDATES, args.view_redundancy))
    if not used:
        parser.error("--select_views goes with --color or --texture T: it chooses the frames "
                     "they take colours from")


def check_candidates(parser, args, frames):
    if requested(args) and len(frames) > MAX_CANDIDATES:
        parser.error("--select_views: %d candidate frames, at most %d; thin them with --start_end "
                     "/ --skip_every" % (len(frames), MAX_CANDIDATES))


def choose(parser, args, mesh, scene, frames, tol):
    """-> the frames the colour or texture step gets: all of them without --select_views, else the
    covering set of the finished mesh, in the order chosen; prints them and the share of vertices
    still short."""
    if not requested(args):
        return frames
    if mesh.empty or not frames:
        parser.error("--select_views: %s" % ("the surface is empty" if mesh.empty else
                                             "--start_end selects no frame of the scene"))
    chosen, gains, short = mesh.best_frames(scene, frames, args.select_views, tol,
                                            redundancy=args.view_redundancy or 1,
                                            return_stats=True)
    if not chosen:
        parser.error("--select_views: none of the %d candidate frames sees the surface" % len(frames))
    print("--select_views: frames %s of %d candidates; %.4f of the %d vertices still short"
          % (",".join(str(i) for i in chosen), len(frames), short / float(len(mesh.vertices)),
             len(mesh.vertices)))
    return chosen
