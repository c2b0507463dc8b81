#!/usr/bin/env python3
"""Ground-truth depth maps of a Restrepo scene from its mesh, on the GPU.

    python -m raynet_amd.scripts.gt_depth_maps SCENE_DIR [--frames 0,1,2]

ray-casts the scene's gt_mesh.obj / gt_mesh.ply (the .obj first) through every pixel of the
chosen frames (all by default) and writes SCENE_DIR/gt/gt_depth_%d.npy ([H, W] float32
distances to the camera centre, 0 where a pixel's ray hits nothing) -- the layout
RestrepoScene, and the reference's `_has_gt_depth` (common/scene.py:179-185), read back.
"""
import argparse
import os
import sys

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description="Write gt/gt_depth_%d.npy of a Restrepo scene by "
                                            "ray-casting its ground-truth mesh")
    p.add_argument("scene_directory", help="Restrepo scene (imgs/, cams_krt/, scene_info.xml, "
                                           "gt_mesh.obj or gt_mesh.ply)")
    p.add_argument("--frames", type=lambda x: [int(f) for f in x.split(",") if f != ""],
                   default=None, help="Comma-separated frame indices (default: all)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
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
