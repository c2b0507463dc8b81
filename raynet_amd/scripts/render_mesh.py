#!/usr/bin/env python3
"""Render a surface mesh from the cameras of a scene, and score it against their photographs.

    python -m raynet_amd.scripts.render_mesh DATASET_DIR MESH.ply OUT_DIR \\
        --dataset_type restrepo --start_end 0,12 [--planes color,depth] [--compare]

MESH.ply is what `fuse_depth_maps` and `render_volume --mesh` write (volume.SurfaceMesh.save_ply).
For every frame of --start_end / --skip_every the mesh is seen from the frame's camera at the
scene's image size, all frames in one launch (volume.SurfaceMesh.render_scene, DESIGN.md section
26), and OUT_DIR gets, of the --planes asked for (a comma-separated list),

    color    render_%03d.png    the vertices' colours interpolated over the faces
    normals  normals_%03d.png   the interpolated unit normals as (n + 1) / 2
    shaded   shaded_%03d.png    a grey headlight image max(0, n . direction to the camera)
    depth    depth_%03d.npy     (H, W) float32, 0 where the ray hits nothing: the wire format
                                compute_metrics reads
    faces    faces_%03d.npy     (H, W) int32 the face hit first, -1 where none, and with it
             bary_%03d.npy      (H, W, 2) float32 where in that face

The default is `color` for a mesh with colours and `shaded` for one without; `color` needs colours
in the file, `normals` and `shaded` compute the normals of a mesh that has none.  --background
R,G,B (0..255) is the colour of the pixels whose rays hit nothing.

--compare scores each `color` render against the frame's image over the pixels the mesh covers
(metrics.photometric_error): one line `view I: coverage C, mae M, psnr P` per frame, and
OUT_DIR/render_metrics.json.

--texture T bakes the selected frames' images (at most 32) into a texture atlas of T texel steps
per chart leg (volume.SurfaceMesh.textured) and writes texture_%03d.png per
frame -- the same render with the atlas looked up at every pixel's face and barycentrics,
bilinear, or the nearest texel with --texture_nearest -- and atlas.png.  --texture_mode and
--texture_normals are the bake's; --texture_tolerance is the slack of its occlusion test in scene
units (default: the median edge length of the mesh).  With --compare every frame gets a second
line `view I texture: coverage C, mae M, psnr P`, and render_metrics.json a list `texture_views`.
"""
import argparse
import json
import os
import sys

import numpy as np

from . import scene_flags, texture_flags, view_flags

PLANES = ("color", "normals", "shaded", "depth", "faces")


def build_parser():
    p = argparse.ArgumentParser(description="Render a surface mesh from a scene's cameras")
    p.add_argument("dataset_directory", help="Directory containing the input data")
    p.add_argument("mesh_file", help="The surface mesh (PLY)")
    p.add_argument("output_directory", help="Directory to save the rendered images")
    p.add_argument("--planes", default=None,
                   help="Comma-separated: %s (default: color if the mesh has colours, else shaded)"
                   % ", ".join(PLANES))
    p.add_argument("--background", default="0,0,0",
                   help="R,G,B (0..255) of the pixels whose rays hit nothing")
    p.add_argument("--compare", action="store_true",
                   help="Score the color renders against the frames' images")
    texture_flags.add_arguments(p, nearest=True)
    view_flags.add_arguments(p)
    p.add_argument("--texture_tolerance", type=float, default=None,
                   help="--texture: the slack of the occlusion test in scene units (default: the "
                        "median edge length of the mesh)")
    scene_flags.add_arguments(p)
    return p


def _median_edge(mesh):
    tri = np.asarray(mesh.vertices, np.float64)[np.asarray(mesh.faces, np.int64)]
    edges = np.concatenate([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]])
    return float(np.median(np.sqrt((edges ** 2).sum(1))))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    scene_flags.check(parser, args)
    texture_flags.check(parser, args)
    view_flags.check(parser, args, used=args.texture is not None)
    if args.texture_tolerance is not None and args.texture is None:
        parser.error("--texture_tolerance goes with --texture T")
    if args.texture_tolerance is not None and not 0.0 <= args.texture_tolerance < float("inf"):
        parser.error("--texture_tolerance takes a finite distance, 0 or more")
    planes = None
    if args.planes is not None:
        planes = [x.strip() for x in args.planes.split(",") if x.strip()]
        unknown = [x for x in planes if x not in PLANES]
        if unknown or not planes:
            parser.error("--planes takes a comma-separated list of %s, got %r"
                         % (", ".join(PLANES), args.planes))
    try:
        background = scene_flags.ints(args.background)
    except ValueError:
        background = ()
    if len(background) != 3 or min(background) < 0 or max(background) > 255:
        parser.error("--background takes three numbers R,G,B in 0..255, got %r" % args.background)
    if args.compare and planes is not None and "color" not in planes:
        parser.error("--compare scores the color renders: add color to --planes")
    if not os.path.isfile(args.mesh_file):
        parser.error("%s: no such file (fuse_depth_maps and render_volume --mesh write one)"
                     % args.mesh_file)
    from raynet_amd.metrics import photometric_error
    from raynet_amd.volume import SurfaceMesh

    mesh = SurfaceMesh.load_ply(args.mesh_file)
    if planes is None:
        planes = ["color" if mesh.colors is not None else "shaded"]
    if "color" in planes and mesh.colors is None:
        parser.error("--planes color: %s has no colours (fuse_depth_maps --color and render_volume "
                     "--mesh --color write them)" % args.mesh_file)
    if args.compare and "color" not in planes:
        parser.error("--compare scores the color renders: %s has no colours" % args.mesh_file)
    if mesh.empty:
        parser.error("%s: the mesh is empty, there is no surface to render" % args.mesh_file)
    scene = scene_flags.open_scene(args)
    frames = scene_flags.frames(parser, args, scene)
    view_flags.check_candidates(parser, args, frames)
    if not view_flags.requested(args):
        texture_flags.check_frames(parser, args, frames)
    if ("normals" in planes or "shaded" in planes) and mesh.normals is None:
        mesh.compute_normals()
    os.makedirs(args.output_directory, exist_ok=True)
    from PIL import Image as PILImage
    cameras = [scene.get_image(i).camera for i in frames]
    rendered = mesh.render_scene(scene, frames)

    def path(pattern, i):
        return os.path.join(args.output_directory, pattern % (i,))

    textured = None
    if args.texture is not None:
        tol = _median_edge(mesh) if args.texture_tolerance is None else args.texture_tolerance
        texture_frames = view_flags.choose(parser, args, mesh, scene, frames, tol)
        texture_flags.check_frames(parser, args, texture_frames)
        baked = texture_flags.bake(parser, args, mesh, scene, texture_frames, tol)
        textured = rendered.textured(baked.with_unseen(), bilinear=not args.texture_nearest)
        baked.save_png(os.path.join(args.output_directory, "atlas.png"))
    scores, texture_scores = [], []
    for k, i in enumerate(frames):
        if "color" in planes:
            PILImage.fromarray(rendered.rgb8(k, background)).save(path("render_%03d.png", i))
        if "normals" in planes:
            PILImage.fromarray(rendered.normal_rgb8(k)).save(path("normals_%03d.png", i))
        if "shaded" in planes:
            PILImage.fromarray(rendered.shaded8(k, cameras)).save(path("shaded_%03d.png", i))
        if "depth" in planes:
            np.save(path("depth_%03d.npy", i), rendered.depth[k].cpu().numpy())
        if "faces" in planes:
            np.save(path("faces_%03d.npy", i), rendered.face[k].cpu().numpy())
            np.save(path("bary_%03d.npy", i), rendered.bary[k].cpu().numpy())
        if args.compare:
            image = np.asarray(scene.get_image(i).image, np.float32)
            color = rendered.color[k].cpu().numpy()
            if image.shape[2] != color.shape[2]:            # a grey photograph
                image = np.repeat(image[:, :, :1], color.shape[2], axis=2)
            score = photometric_error(color, image, rendered.mask[k].cpu().numpy())
            print("view %d: coverage %.4f, mae %.4f, psnr %.2f"
                  % (i, score["coverage"], score["mae"], score["psnr"]))
            scores.append(dict(view=i, **score))
        if textured is not None:
            PILImage.fromarray(textured.rgb8(k, background)).save(path("texture_%03d.png", i))
        if textured is not None and args.compare:
            color = textured.color[k].cpu().numpy()
            if image.shape[2] != color.shape[2]:
                image = np.repeat(image[:, :, :1], color.shape[2], axis=2)
            score = photometric_error(color, image, rendered.mask[k].cpu().numpy())
            print("view %d texture: coverage %.4f, mae %.4f, psnr %.2f"
                  % (i, score["coverage"], score["mae"], score["psnr"]))
            texture_scores.append(dict(view=i, **score))
    if args.compare:
        with open(os.path.join(args.output_directory, "render_metrics.json"), "w") as f:
            json.dump(dict(mesh=os.path.basename(args.mesh_file), faces=int(len(mesh.faces)),
                           views=scores, **({} if textured is None else
                                            dict(texture_views=texture_scores))), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
