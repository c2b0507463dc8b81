"""From photographs to a textured mesh and its score, through the command lines (DESIGN.md section
27): the two-sphere scene of the chain tests with photographs whose colour is a periodic function
of the 3-D point a pixel sees, fused, cleaned and simplified to cells of two voxel sides, coloured
per vertex and textured, then rendered both ways and scored against the photographs it was baked
from.

PERIOD, PHASE and T were chosen on the CPU with the restatements (fusion_truth, isosurface_truth,
components_truth, simplify_truth, appearance_truth, render_truth, texture_truth run as this chain;
the images are the scene's 20 x 30): the simplified mesh has 93 faces, a vertex stands for about
2.2 pixels, and a period of 0.4 scene units is about 4 pixels.  There the restatements give, per
view, a PSNR of 13.82, 13.34 and 14.64 dB with vertex colours and 16.61, 18.24 and 22.51 dB with
the texture at T = 4 (15.28, 17.13, 18.75 at T = 2; 16.97, 18.67, 23.92 at T = 8): at least 2.8 dB
in every view.  The test asserts the relation only."""
import json
import os
import re

import numpy as np
import pytest

import mesh_harness as h
import raycast_truth as rt

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
PERIOD, PHASE, T = 0.4, (0.0, 1.0, 2.0), 4


def _photograph(cam, H, W, maps):
    """(H, W, 3) uint8: the two spheres as the camera sees them, the colour 0.5 + 0.4 sin(2 pi p /
    PERIOD + PHASE) of the 3-D point p the pixel's ray hits (from the analytic depth), grey 51
    where it hits nothing."""
    ys, xs = np.mgrid[0:H, 0:W]
    o, dst = rt.pixel_rays(cam.P_pinv, cam.center, xs.reshape(-1), ys.reshape(-1))
    ray = dst.astype(D) - o.astype(D)
    ray /= np.linalg.norm(ray, axis=1)[:, None]
    point = o.astype(D) + maps.reshape(-1, 1).astype(D) * ray
    colour = 0.5 + 0.4 * np.sin(2 * np.pi * point / PERIOD + np.array(PHASE))
    colour[maps.reshape(-1) <= 0] = 0.2
    return np.rint(colour * 255).astype(np.uint8).reshape(H, W, 3)


def _read_obj(path):
    v, vt, f, mtllib = [], [], [], None
    for line in open(path).read().splitlines():
        word = line.split()
        if word and word[0] == "v":
            v.append([float(x) for x in word[1:]])
        elif word and word[0] == "vt":
            vt.append([float(x) for x in word[1:]])
        elif word and word[0] == "f":
            f.append([[int(k) for k in corner.split("/")] for corner in word[1:]])
        elif word and word[0] == "mtllib":
            mtllib = word[1]
    return np.array(v, F), np.array(vt, D), np.array(f), mtllib


def test_from_photographs_to_a_textured_mesh_that_beats_its_vertex_colours(tmp_path, capsys):
    from PIL import Image as PILImage
    from raynet_amd import texture as tx
    from raynet_amd.scripts import fuse_depth_maps, render_mesh
    from raynet_amd.volume import SurfaceMesh
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps()
    scene_dir, preds, out = str(tmp_path / "scene"), str(tmp_path / "predictions"), str(tmp_path / "out")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    for i, (cam, d) in enumerate(zip(cams, gt_maps)):
        PILImage.fromarray(_photograph(cam, H, W, d)).save(
            os.path.join(scene_dir, "imgs", "frame_%03d.png" % i))
    os.makedirs(preds)
    ply = str(tmp_path / "mesh.ply")
    assert fuse_depth_maps.main([scene_dir, preds, ply, "--gt", "--truncation", "0.25", "--start_end",
                                 "0,3", "--grid_shape", "18,22,14", "--keep_largest", "1",
                                 "--simplify", "2", "--color", "--texture", str(T)]) == 0
    capsys.readouterr()
    # the OBJ triple beside the mesh file, with its stem: the PLY's surface, one chart per face
    mesh = SurfaceMesh.load_ply(ply)
    obj, mtl, png = (str(tmp_path / ("mesh." + ext)) for ext in ("obj", "mtl", "png"))
    v, vt, f, mtllib = _read_obj(obj)
    assert mtllib == "mesh.mtl" and "map_Kd mesh.png" in open(mtl).read()
    assert np.array_equal(v, mesh.vertices) and np.array_equal(f[..., 0] - 1, mesh.faces)
    layout = tx.atlas_layout(len(mesh.faces), T)
    assert np.array_equal(vt[f[..., 1] - 1], tx.face_uvs(len(mesh.faces), layout))
    atlas = np.asarray(PILImage.open(png))
    assert atlas.shape == (layout.Ht, layout.Wt, 3)
    owned = tx.owned_texels(layout)
    assert (atlas[~owned] == 0).all() and atlas[owned].std() > 20
    # both renders against the photographs they were made from
    diagonal = float(np.sqrt(((2.0 / np.array(grid, D)) ** 2).sum()))
    assert render_mesh.main([scene_dir, ply, out, "--start_end", "0,3", "--compare", "--background",
                             "51,51,51", "--texture", str(T), "--texture_tolerance",
                             "%.17g" % diagonal]) == 0
    printed = capsys.readouterr().out.strip().split("\n")
    scores = json.load(open(os.path.join(out, "render_metrics.json")))
    assert len(scores["views"]) == 3 and len(scores["texture_views"]) == 3 and len(printed) == 6
    assert np.array_equal(np.asarray(PILImage.open(os.path.join(out, "atlas.png"))).shape, atlas.shape)
    for i in range(3):
        s, t = scores["views"][i], scores["texture_views"][i]
        assert printed[2 * i] == "view %d: coverage %.4f, mae %.4f, psnr %.2f" % (
            i, s["coverage"], s["mae"], s["psnr"])
        assert printed[2 * i + 1] == "view %d texture: coverage %.4f, mae %.4f, psnr %.2f" % (
            i, t["coverage"], t["mae"], t["psnr"])
        assert re.match(r"^view \d+ texture: ", printed[2 * i + 1])
        for pattern in ("render_%03d.png", "texture_%03d.png"):
            assert os.path.isfile(os.path.join(out, pattern % i)), pattern % i
        assert t["view"] == s["view"] == i and t["coverage"] == s["coverage"] > 0
        print("view %d: %d faces, psnr %.2f dB with vertex colours, %.2f dB with the texture at T = %d"
              % (i, len(mesh.faces), s["psnr"], t["psnr"], T))
        assert t["psnr"] > s["psnr"]


def test_render_volume_writes_the_triple_beside_its_mesh(tmp_path, capsys):
    """render_volume --mesh --texture on a ball of belief in the two-sphere scene's box, with the
    sub-flags: the OBJ triple of the PLY's surface, the atlas seen by some view."""
    from PIL import Image as PILImage
    from raynet_amd import texture as tx
    from raynet_amd.scripts import render_volume
    from raynet_amd.volume import OccupancyVolume, SurfaceMesh
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps()
    scene_dir, out = str(tmp_path / "scene"), str(tmp_path / "out")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    for i, (cam, d) in enumerate(zip(cams, gt_maps)):
        PILImage.fromarray(_photograph(cam, H, W, d)).save(
            os.path.join(scene_dir, "imgs", "frame_%03d.png" % i))
    axes = [np.linspace(-1, 1, 2 * g + 1)[1::2] for g in grid]           # the voxel centres
    x, y, z = np.meshgrid(*axes, indexing="ij")
    radius = np.sqrt(x ** 2 + y ** 2 + (z + 0.1) ** 2)
    belief = (1.0 / (1.0 + np.exp((radius - 0.5) / 0.05))).astype(F)
    occupancy = str(tmp_path / "occupancy.npz")
    OccupancyVolume(belief, bbox, grid).save(occupancy)
    ply = str(tmp_path / "ball.ply")
    assert render_volume.main([scene_dir, occupancy, out, "--start_end", "0,3", "--mesh", ply,
                               "--simplify", "2", "--texture", "2", "--texture_mode", "best",
                               "--texture_normals", "vertex"]) == 0
    capsys.readouterr()
    mesh = SurfaceMesh.load_ply(ply)
    v, vt, f, mtllib = _read_obj(str(tmp_path / "ball.obj"))
    assert mtllib == "ball.mtl" and "map_Kd ball.png" in open(str(tmp_path / "ball.mtl")).read()
    assert len(mesh.faces) > 20 and np.array_equal(v, mesh.vertices)
    assert np.array_equal(f[..., 0] - 1, mesh.faces)
    layout = tx.atlas_layout(len(mesh.faces), 2)
    assert np.array_equal(vt[f[..., 1] - 1], tx.face_uvs(len(mesh.faces), layout))
    atlas = np.asarray(PILImage.open(str(tmp_path / "ball.png")))
    owned = tx.owned_texels(layout)
    assert atlas.shape == (layout.Ht, layout.Wt, 3) and (atlas[~owned] == 0).all()
    # texels no view saw are the grey of `unseen`; the others carry the photographs' waves
    assert (atlas[owned] != 128).any(1).sum() > owned.sum() // 4
