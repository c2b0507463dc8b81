#!/usr/bin/env python3
"""Ground-truth depth maps of a scene from what its dataset ships, on the GPU.

    python -m raynet_amd.scripts.gt_depth_maps SCENE_DIR [--frames 0,1,2]

ray-casts a Restrepo scene's gt_mesh.obj / gt_mesh.ply (the .obj first) through every pixel of the
chosen frames (all by default) and writes SCENE_DIR/gt/gt_depth_%d.npy ([H, W] float32
distances to the camera centre, 0 where a pixel's ray hits nothing) -- the layout
RestrepoScene, and the reference's `_has_gt_depth` (common/scene.py:179-185), read back.

    python -m raynet_amd.scripts.gt_depth_maps DATASET_DIR --dataset_type dtu --scene_idx N
        [--closing_radius S --slope_gain K --tau_px T]

renders a DTU scan's point cloud Points/stl/stlNNN_total.ply into every frame (DESIGN.md section
14b) and writes DATASET_DIR/Depth/scanNNN/depth_%03d.npy ([H, W] float32 z-depths, 0 where a
pixel has no ground truth) -- the layout DTUScene reads back.  The maps are only as good as the
cloud is dense: below about one point per pixel footprint more and more pixels stay empty.
"""
import argparse
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(
        description="Write the ground-truth depth maps of a scene: gt/gt_depth_%%d.npy of a "
                    "Restrepo scene by ray-casting its mesh, or Depth/scanNNN/depth_%%03d.npy of "
                    "a DTU scan by rendering its point cloud (only as good as the cloud is dense: "
                    "below about one point per pixel footprint pixels stay empty)")
    p.add_argument("scene_directory", help="Restrepo scene (imgs/, cams_krt/, scene_info.xml, "
                                           "gt_mesh.obj or gt_mesh.ply), or the DTU dataset "
                                           "directory with --dataset_type dtu")
    p.add_argument("--frames", type=lambda x: [int(f) for f in x.split(",") if f != ""],
                   default=None, help="Comma-separated frame indices (default: all; Restrepo only)")
    p.add_argument("--dataset_type", choices=("restrepo", "dtu"), default="restrepo")
    p.add_argument("--scene_idx", type=int, default=None, help="The DTU scan's number")
    p.add_argument("--illumination", default="max",
                   help="The DTU illumination whose images name the frames (default: max)")
    p.add_argument("--closing_radius", type=int, default=1,
                   help="DTU: window radius S of the hidden-point filter in pixels, 0 = no filter "
                        "(default: 1)")
    p.add_argument("--slope_gain", type=float, default=1.5,
                   help="DTU: tolerance per unit of depth slope over the window (default: 1.5)")
    p.add_argument("--tau_px", type=float, default=1.0,
                   help="DTU: depth tolerance in pixel footprints (default: 1.0)")
    return p


def _main_dtu(args):
    if args.scene_idx is None:
        raise SystemExit("--dataset_type dtu needs --scene_idx")
    if args.frames is not None:
        # DTUScene pairs the i-th sorted file of Depth/scanNNN with the i-th image: a subset of
        # the frames on disk would be read back as other frames
        raise SystemExit("--frames is not supported with --dataset_type dtu: the loader pairs the "
                         "i-th depth file with the i-th image, so every frame is written")
    from raynet_amd.common.scene import DTUScene
    scene = DTUScene(args.scene_directory, args.scene_idx, illumination=args.illumination)
    if not os.path.isfile(scene._gt_stl_path):
        raise SystemExit("no point cloud %s" % scene._gt_stl_path)
    renderer = scene._get_cloud_renderer()
    os.makedirs(scene._depth_dir, exist_ok=True)
    for i in range(scene.n_images):
        im = scene.get_image(i)
        Z = renderer.depth_maps([im.camera], im.height, im.width,
                                closing_radius=args.closing_radius, slope_gain=args.slope_gain,
                                tau_px=args.tau_px)[0].cpu().numpy()
        # named after the image's own number (rect_007_max.png -> depth_007.npy): the same order
        number = int(os.path.basename(scene._image_paths[i]).split(".")[0].split("_")[1])
        np.save(os.path.join(scene._depth_dir, "depth_%03d.npy" % number), Z)
        print("frame %d: %d of %d pixels filled" % (i, int((Z != 0).sum()), Z.size))
    return 0


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.dataset_type == "dtu":
        return _main_dtu(args)
    from raynet_amd.common.scene import RestrepoScene
    scene = RestrepoScene(args.scene_directory)
    frames = range(scene.n_images) if args.frames is None else args.frames
    raycaster = scene._get_raycaster()
    out_dir = os.path.join(args.scene_directory, "gt")
    os.makedirs(out_dir, exist_ok=True)
    for i in frames:
        if not 0 <= i < scene.n_images:
            raise SystemExit("frame %d: the scene has %d frames" % (i, scene.n_images))
        im = scene.get_image(i)
        D = raycaster.depth_map(im.camera, im.height, im.width).cpu().numpy()
        np.save(os.path.join(out_dir, "gt_depth_%d.npy" % i), D)
        print("frame %d: %d of %d pixels hit the mesh" % (i, int((D != 0).sum()), D.size))
    return 0


if __name__ == "__main__":
    sys.exit(main())
