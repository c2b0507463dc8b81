#!/usr/bin/env python3
"""Fuse depth maps into a surface mesh.

    python -m raynet_amd.scripts.fuse_depth_maps DATASET_DIR PREDICTIONS_DIR OUT.ply \\
        --dataset_type restrepo --start_end 0,12 --grid_shape 256,256,128 [--confidence_weights]

PREDICTIONS_DIR holds `depth_%03d.npy` (--pred_suffix), one (H, W) map of distances to the camera
centre per frame of --start_end / --skip_every: what `raynet_amd.scripts.forward_pass` writes, with
any factory -- the MV-CNN paths, which have no occupancy volume, included.  The maps are fused into
a truncated signed distance volume over --grid_shape voxels of the scene's bounding box
(raynet_amd.fusion) and the zero level of that volume is written to OUT.ply,
the binary PLY common.mesh_io.parse_gt_data_from_ply reads back.  The surface is open where
observation ends.

--truncation T       the truncation distance in scene units (default: 3 voxel sides)
--border B           pixels to stay away from the edge of the depth maps (default 0)
--min_weight M       a voxel belongs to the surface only if the weights of the views that saw it
                     sum to at least M (default 0: one view is enough)
--confidence_weights weigh every pixel with PREDICTIONS_DIR/confidence_%03d.npy, what
                     `forward_pass --depth_statistics` writes; --min_confidence X: pixels whose
                     confidence is below X do not count at all
--gt                 fuse the scene's ground-truth depth maps instead (PREDICTIONS_DIR is not
                     read): the ground-truth MESH of a scene that ships none, DTU's for instance,
                     for the surface_accuracy / surface_completeness metrics
--min_consistent_views K [--max_violations M --consistency_abs X --consistency_rel X]
                     before the fusion, drop every pixel that fewer than K of the other frames
                     agree with or that more than M frames see past, within X + X * depth
                     (raynet_amd.scripts.consistency_flags); a line per frame
                     says how many pixels went, as disagreeing or as violating
--volume OUT.npz     also save the volume (fusion.TSDFVolume.load reads it back)
--normals, --color   the mesh file also carries vertex normals / the colours of the frames' images
                     (volume.SurfaceMesh.compute_normals / .colorize; at most 32 frames)
--select_views K [--view_redundancy R]
                     every frame (at most 64) is fused, but --color / --texture get only the
                     K <= 32 frames that between them see the most of the finished surface
                     (raynet_amd.scripts.view_flags); a line says which
--mesh_cloud PATH --mesh_samples N [--seed S]
                     also write N area-weighted points of the surface as a point cloud, the form
                     compute_metrics scores
the mesh-cleanup flags
                     drop the floaters (--min_component_faces, --min_component_fraction,
                     --keep_largest), then cap the small holes (--fill_holes N), then
                     --simplify the surface, then --smooth it, before
                     normals, colours and --mesh_cloud: see raynet_amd.scripts.mesh_flags
"""
import argparse
import sys

import numpy as np

from . import consistency_flags, mesh_flags, scene_flags, texture_flags, view_flags


def build_parser():
    p = argparse.ArgumentParser(description="Fuse depth maps into a TSDF volume and a surface mesh")
    p.add_argument("dataset_directory", help="Directory containing the input data")
    p.add_argument("predictions_directory", help="Directory of the depth maps (depth_%%03d.npy)")
    p.add_argument("output_mesh", help="The PLY file to write the surface to")
    p.add_argument("--grid_shape", type=scene_flags.ints, default="256,256,128")
    p.add_argument("--truncation", type=float, default=None,
                   help="The truncation distance in scene units (default: 3 voxel sides)")
    p.add_argument("--min_weight", type=float, default=0.0,
                   help="The least sum of weights a voxel of the surface must have")
    p.add_argument("--border", type=float, default=0.0,
                   help="Pixels to stay away from the edge of the depth maps")
    p.add_argument("--pred_suffix", default="depth",
                   help="The suffix for the predicted files (default=depth)")
    p.add_argument("--confidence_weights", action="store_true",
                   help="Weigh the pixels with confidence_%%03d.npy of forward_pass --depth_statistics")
    p.add_argument("--min_confidence", type=float, default=None,
                   help="--confidence_weights: pixels whose confidence is below this do not count")
    p.add_argument("--gt", action="store_true",
                   help="Fuse the scene's ground-truth depth maps instead of predictions")
    p.add_argument("--volume", default=None, help="Also save the TSDF volume (.npz) here")
    p.add_argument("--normals", action="store_true", help="With vertex normals")
    p.add_argument("--color", action="store_true",
                   help="With vertex normals and the colours of the frames' images")
    mesh_flags.add_cloud_arguments(p)
    mesh_flags.add_arguments(p)
    texture_flags.add_arguments(p)
    view_flags.add_arguments(p)
    consistency_flags.add_arguments(p)
    scene_flags.add_arguments(p)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    if isinstance(args.grid_shape, str):
        args.grid_shape = scene_flags.ints(args.grid_shape)
    if len(args.grid_shape) != 3 or min(args.grid_shape) < 1:
        parser.error("--grid_shape takes three positive sizes, GX,GY,GZ")
    if args.truncation is not None and not 0.0 < args.truncation < float("inf"):
        parser.error("--truncation takes a positive, finite distance")
    if not 0.0 <= args.border < float("inf"):
        parser.error("--border takes a finite number of pixels, 0 or more")
    if not args.min_weight >= 0.0:
        parser.error("--min_weight takes a number that is 0 or more")
    mesh_flags.check_cloud(parser, args)
    if args.min_confidence is not None and not args.confidence_weights:
        parser.error("--min_confidence goes with --confidence_weights")
    if args.gt and args.confidence_weights:
        parser.error("--confidence_weights: ground-truth depth maps have no confidence")
    mesh_flags.check(parser, args)
    texture_flags.check(parser, args)
    view_flags.check(parser, args, used=bool(args.color or args.texture is not None))
    consistency_flags.check(parser, args)
    if args.gt and consistency_flags.requested(args):
        parser.error("--min_consistent_views: ground-truth depth maps are not checked")
    from raynet_amd.fusion import fuse_scene

    scene = scene_flags.open_scene(args)
    frames = scene_flags.frames(parser, args, scene)
    view_flags.check_candidates(parser, args, frames)
    if not view_flags.requested(args):
        texture_flags.check_color_frames(parser, args, frames)
        texture_flags.check_frames(parser, args, frames)
    consistency_flags.check_frames(parser, args, frames)
    weights = None
    if args.gt:
        depth_maps = [scene.get_depth_map(i) for i in frames]
    else:
        depth_maps = scene_flags.load_maps(parser, args.predictions_directory, args.pred_suffix,
                                           frames)
        if args.confidence_weights:
            weights = [np.asarray(w, np.float32) for w in scene_flags.load_maps(
                parser, args.predictions_directory, "confidence", frames)]
            if args.min_confidence is not None:
                weights = [np.where(w >= np.float32(args.min_confidence), w, np.float32(0))
                           for w in weights]
    if consistency_flags.requested(args):
        depth_maps = consistency_flags.filter_maps(args, scene, frames, depth_maps, args.border)
    volume = fuse_scene(scene, depth_maps, frames, args.grid_shape, trunc=args.truncation,
                        weights=weights, border=args.border)
    if args.volume:
        volume.save(args.volume)
    mesh = mesh_flags.apply(volume.mesh(args.min_weight), args, volume)
    if (args.normals or args.color or args.mesh_cloud or args.texture is not None) and mesh.empty:
        parser.error("the fused surface is empty: no voxel pair straddles a measured depth")
    if args.normals or args.color:
        mesh.compute_normals()
    color_frames = frames
    if view_flags.requested(args):
        color_frames = view_flags.choose(parser, args, mesh, scene, frames,
                                         mesh_flags.voxel_diagonal(volume))
        texture_flags.check_color_frames(parser, args, color_frames)
        texture_flags.check_frames(parser, args, color_frames)
    if args.color:
        mesh.colorize(scene, color_frames, tol=mesh_flags.voxel_diagonal(volume))
    mesh.save_ply(args.output_mesh)
    if args.texture is not None:
        texture_flags.write(parser, args, mesh, scene, color_frames,
                            mesh_flags.voxel_diagonal(volume), args.output_mesh)
    if args.mesh_cloud:
        mesh.pointcloud(args.mesh_samples, args.seed).save_ply(args.mesh_cloud)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
