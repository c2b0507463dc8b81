#!/usr/bin/env python3
"""Render a saved occupancy volume from the cameras of a scene, and export its voxel cloud.

    python -m raynet_amd.scripts.render_volume DATASET_DIR OCCUPANCY.npz OUT_DIR \\
        --dataset_type restrepo --start_end 0,12 [--plane expected_depth] [--ply cloud.ply]

OCCUPANCY.npz is what `raynet_amd.scripts.forward_pass --save_occupancy` writes.  For every frame
of --start_end / --skip_every (the forward pass's own indexing -- but the frames need not be the
ones the pass ran over: a held-out view renders like any other) the volume is rendered from the
frame's camera (volume.OccupancyVolume.render) and OUT_DIR gets

    depth_%03d.npy     the chosen --plane, (H, W) float32: the wire format compute_metrics and
                       convert_to_pointcloud read
    opacity_%03d.npy   how much of the ray the volume stops, (H, W) float32 in [0, 1]

--ply PATH writes the centres of the voxels whose occupancy is at least --threshold as a point
cloud: the surface voxels (those with a free or missing 6-neighbour), or with --all_voxels every
one of them.

--mesh PATH writes the surface of the volume at --threshold as a triangle mesh (a binary PLY;
volume.OccupancyVolume.mesh: marching tetrahedra, interpolated between the voxel centres), closed
where the occupied region meets the border of the grid unless --open is given.  --mesh_cloud PATH
--mesh_samples N [--seed S] writes N area-weighted points of that surface as a point cloud, the
form compute_metrics scores.

--color, with --mesh: the mesh file also carries vertex normals and the colours of the images of
the frames of --start_end / --skip_every (at most 32; volume.SurfaceMesh.colorize).  A frame
colours the vertices that face it and that the mesh itself does not hide from it; --color_mode
blend (default) takes the cos^2-weighted mean of the frames, best the frame that faces a vertex
best.  --depth_tolerance is the slack of the occlusion test in voxel diagonals (default 1: a
vertex lies on an edge of a lattice cell, and the surface point its nearest pixel records lies in
the same or the next cell unless the view is grazing).

The mesh-cleanup flags, with --mesh: drop the floaters (--min_component_faces,
--min_component_fraction, --keep_largest), then cap the small holes (--fill_holes N), then
--simplify the surface, then --smooth it, before
colours and --mesh_cloud: see raynet_amd.scripts.mesh_flags.
"""
import argparse
import os
import sys

import numpy as np

from . import mesh_flags, scene_flags, texture_flags, view_flags

PLANES = ["depth", "expected_depth", "median_depth"]


def build_parser():
    p = argparse.ArgumentParser(description="Render an occupancy volume from a scene's cameras")
    p.add_argument("dataset_directory", help="Directory containing the input data")
    p.add_argument("occupancy_file", help="The occupancy.npz of a forward pass (--save_occupancy)")
    p.add_argument("output_directory", help="Directory to save the rendered maps")
    p.add_argument("--plane", choices=PLANES, default="depth",
                   help="Which depth goes to depth_%%03d.npy")
    p.add_argument("--ply", default=None, help="Also write the cloud of occupied voxels here")
    p.add_argument("--threshold", type=float, default=0.5,
                   help="--ply: a voxel is occupied when its probability is at least this")
    p.add_argument("--all_voxels", action="store_true",
                   help="--ply: every occupied voxel, not only those on the surface")
    p.add_argument("--mesh", default=None,
                   help="Also write the surface at --threshold as a triangle mesh (PLY) here")
    p.add_argument("--open", action="store_true",
                   help="--mesh / --mesh_cloud: leave the surface open at the border of the grid")
    mesh_flags.add_cloud_arguments(p)
    p.add_argument("--color", action="store_true",
                   help="--mesh: with vertex normals and the colours of the frames' images")
    p.add_argument("--color_mode", choices=["blend", "best"], default="blend",
                   help="--color: the weighted mean of the frames that see a vertex, or the best one")
    p.add_argument("--depth_tolerance", type=float, default=1.0,
                   help="--color: the slack of the occlusion test, in voxel diagonals")
    mesh_flags.add_arguments(p)
    texture_flags.add_arguments(p)
    view_flags.add_arguments(p)
    scene_flags.add_arguments(p)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    mesh_flags.check_cloud(parser, args)
    if (args.mesh or args.mesh_cloud) and not 0.0 < args.threshold <= 1.0:
        parser.error("--mesh / --mesh_cloud: --threshold must lie in (0, 1]")
    if args.color and not args.mesh:
        parser.error("--color goes with --mesh PATH: the colours are the mesh's")
    if not (args.depth_tolerance >= 0.0 and args.depth_tolerance < float("inf")):
        parser.error("--depth_tolerance takes a finite number of voxel diagonals, 0 or more")
    mesh_flags.check(parser, args, mesh_requested=bool(args.mesh))
    texture_flags.check(parser, args, mesh_requested=bool(args.mesh))
    view_flags.check(parser, args,
                     used=bool(args.mesh) and (args.color or args.texture is not None))
    if not os.path.isfile(args.occupancy_file):
        parser.error("%s: no such file (forward_pass --save_occupancy writes it)"
                     % args.occupancy_file)
    from raynet_amd.volume import OccupancyVolume

    volume = OccupancyVolume.load(args.occupancy_file)
    scene = scene_flags.open_scene(args)
    os.makedirs(args.output_directory, exist_ok=True)
    # (no frame is no error here: --ply and --mesh need none; --color says so itself, below)
    frames = scene_flags.frames(parser, args, scene, required=False)
    view_flags.check_candidates(parser, args, frames)
    if not view_flags.requested(args):
        texture_flags.check_color_frames(parser, args, frames)
        texture_flags.check_frames(parser, args, frames)
    for i, r in zip(frames, volume.render_scene(scene, frames)):
        np.save(os.path.join(args.output_directory, "depth_%03d.npy" % (i,)),
                getattr(r, args.plane))
        np.save(os.path.join(args.output_directory, "opacity_%03d.npy" % (i,)), r.opacity)
    if args.ply:
        volume.pointcloud(args.threshold, surface_only=not args.all_voxels).save_ply(args.ply)
    if args.mesh or args.mesh_cloud:
        mesh = mesh_flags.apply(volume.mesh(args.threshold, closed=not args.open), args, volume)
        tol = args.depth_tolerance * mesh_flags.voxel_diagonal(volume)
        color_frames = frames
        if args.mesh and view_flags.requested(args):
            color_frames = view_flags.choose(parser, args, mesh, scene, frames, tol)
            texture_flags.check_color_frames(parser, args, color_frames)
            texture_flags.check_frames(parser, args, color_frames)
        if args.mesh and args.color:
            if mesh.empty or not color_frames:
                parser.error("--color: %s" % ("the surface is empty" if mesh.empty else
                                              "--start_end selects no frame of the scene"))
            mesh.compute_normals()
            mesh.colorize(scene, color_frames, tol=tol, mode=args.color_mode)
        if args.mesh:
            mesh.save_ply(args.mesh)
        if args.mesh and args.texture is not None:
            texture_flags.write(parser, args, mesh, scene, color_frames, tol, args.mesh)
        if args.mesh_cloud:
            if mesh.empty:
                parser.error("no voxel reaches --threshold %g: the surface is empty and has no "
                             "points to sample" % args.threshold)
            mesh.pointcloud(args.mesh_samples, args.seed).save_ply(args.mesh_cloud)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
