#!/usr/bin/env python3
"""What normals and colours cost: rn_vertex_area_normals against the bytes
it has to move at the bandwidth rn_occupancy_grid -- one streaming pass over the volume, the
yardstick of section 19 -- reaches in the same process, and rn_project_colors (blend and best)
against V calls of rn_consistency_tau on the same points and depth maps: the same fp64 projection
and one gather per view, with no colour.  One process on one GPU; prints one JSON line and writes
it to profiles/appearance_bench.json.

The mesh is the synthetic scene's after one forward pass at bench.py's shape (5 views of 480 x
640, 64 planes, 128^3 voxels, M = 384), closed, at threshold 0.5; the images are 5 views of 480 x
640 x 3 random floats on the scene's cameras, the occluders the mesh's own depth maps, the
tolerance one voxel diagonal.  The launches take turns; per launch a hipEvent pair on the stream
(rn_timer_*), after `--warmup` launches of each, min and median over `--repeats`.

    python tools/appearance_bench.py [--repeats 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, V, NEIGHBORS, D, M, GRID, C = 480, 640, 5, 4, 64, 384, (128, 128, 128), 3
THRESHOLD = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "appearance_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.appearance import corner_table, pack_cameras
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.synthetic import make_synthetic_scene
    _lib.build()

    scene, bank = make_synthetic_scene(H=H, W=W, n_views=V, focal=1.5 * H, seed=1234)
    gp = GenerationParameters(depth_planes=D, neighbors=NEIGHBORS,
                              grid_shape=np.array(GRID, np.int32),
                              max_number_of_marched_voxels=M, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    for out in fp.forward_pass(scene, (0, V, 1)):
        del out
    volume = fp.occupancy_volume()
    ctx = volume._context((1, 1), None)
    mesh = volume.mesh(THRESHOLD, closed=True)
    nv, nf = len(mesh.vertices), len(mesh.faces)
    dev = ctx.device
    vertices = torch.from_numpy(mesh.vertices).to(dev)
    faces = torch.from_numpy(mesh.faces).to(dev)
    offsets, corners = corner_table(faces, nv)
    area = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    ctx.vertex_area_normals(vertices, faces, offsets, corners, area)
    normals = torch.nn.functional.normalize(area.double(), dim=1).float().contiguous()

    cams = [scene.get_image(i).camera for i in range(V)]
    cameras = torch.from_numpy(pack_cameras(cams)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    images = torch.rand((V, H, W, C), generator=g).to(dev)
    caster = mesh.raycaster()
    depths = torch.stack([caster.depth_map(cam, H, W) for cam in cams]).contiguous()
    bbox = volume.bbox.astype(np.float64)
    tol = float(np.sqrt((((bbox[3:] - bbox[:3]) / np.array(GRID)) ** 2).sum()))
    colors = torch.empty((nv, C), dtype=torch.float32, device=dev)
    weight = torch.empty((nv,), dtype=torch.float32, device=dev)
    views = torch.empty((nv,), dtype=torch.int32, device=dev)

    # the yardstick's inputs: the same points as (3, n) float64, P and centre per view
    points64 = vertices.double().t().contiguous()
    Ps = [torch.from_numpy(np.ascontiguousarray(cam.P, np.float64)).to(dev) for cam in cams]
    centres = [torch.from_numpy(np.asarray(cam.center, np.float64).reshape(4)).to(dev) for cam in cams]
    tau = torch.empty((nv,), dtype=torch.float64, device=dev)

    def consistency():
        for k in range(V):
            ctx.consistency_tau(H, W, k == 0, points64, Ps[k], centres[k], depths[k], tau)

    def project(mode, with_depths=True, with_normals=True):
        ctx.project_colors(vertices, normals if with_normals else None, cameras, images,
                           depths if with_depths else None, tol, 0.0, 0.0, mode, colors, weight,
                           views)

    acc_grid = fp.accumulator.contiguous()
    bel = torch.empty(GRID, dtype=torch.float32, device=dev)
    launches = {
        "occupancy_grid": lambda: fp._ctx.occupancy_grid(acc_grid, False, 0.0, bel),
        "vertex_area_normals": lambda: ctx.vertex_area_normals(vertices, faces, offsets, corners, area),
        "project_colors_blend": lambda: project(0),
        "project_colors_best": lambda: project(1),
        "project_colors_no_depths_no_normals": lambda: project(0, False, False),
        "consistency_tau_x%d" % V: consistency,
    }
    for _ in range(args.warmup):
        for f in launches.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in launches}
    for _ in range(args.repeats):
        for k, f in launches.items():
            ctx.timer_start()
            f()
            ms[k].append(ctx.timer_stop())
    torch.cuda.synchronize()
    project(0)
    torch.cuda.synchronize()
    mask = views.cpu().numpy().view(np.uint32)
    uniq, inverse = np.unique(mask, return_inverse=True)
    seen_by = np.bincount(np.array([bin(m).count("1") for m in uniq])[inverse], minlength=V + 1)

    G = GRID[0] * GRID[1] * GRID[2]
    normal_bytes = {"vertices": 12 * nv, "faces": 12 * nf, "offsets": 4 * (nv + 1),
                    "corners": 12 * nf, "normals_written": 12 * nv}
    res = {"tool": "appearance_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup,
           "shape": dict(grid=GRID, threshold=THRESHOLD, views=V, H=H, W=W, C=C, D=D, M=M,
                         tol=round(tol, 6)),
           "nv": nv, "nf": nf, "vertices_seen_by_k_views": seen_by.tolist()}
    for k in launches:
        med = float(np.median(ms[k]))
        res[k] = {"ms_min": round(float(min(ms[k])), 4), "ms_median": round(med, 4),
                  "ms_max": round(float(max(ms[k])), 4)}
    yard = 8 * G / (res["occupancy_grid"]["ms_median"] * 1e-3)
    res["occupancy_grid"]["GB_per_s"] = round(yard / 1e9, 1)
    total = sum(normal_bytes.values())
    at_yardstick = total / yard * 1e3
    res["vertex_area_normals"].update(
        bytes=dict(normal_bytes, total=total),
        GB_per_s=round(total / (res["vertex_area_normals"]["ms_median"] * 1e-3) / 1e9, 1),
        ms_at_yardstick_bandwidth=round(at_yardstick, 4),
        ratio_to_that=round(res["vertex_area_normals"]["ms_median"] / at_yardstick, 2))
    yard_ms = res["consistency_tau_x%d" % V]["ms_median"]
    for k in ("project_colors_blend", "project_colors_best", "project_colors_no_depths_no_normals"):
        res[k]["ratio_to_consistency_tau"] = round(res[k]["ms_median"] / yard_ms, 2)
        res[k]["ns_per_vertex_view"] = round(res[k]["ms_median"] * 1e6 / (nv * V), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
