#!/usr/bin/env python3
"""What fusing depth maps costs: rn_tsdf_integrate against
rn_project_colors on the same G voxel centres with the same V cameras and depth maps (C = 1, no
normals: the same fp64 projection per point and view, and a bilinear fetch of four pixels next to
the depth lookup where the fusion has a single gather), and the whole fuse -> mesh() against the
forward pass that made the maps.  One process on one GPU; prints one JSON line and writes it to
profiles/fusion_bench.json.

The maps are the synthetic scene's after one forward pass with statistics at bench.py's shape (5
views of 480 x 640, 64 planes, 128^3 voxels, M = 384); they are fused into that grid and into the
command line's default grid, 256 x 256 x 128.  The launches take turns; per launch a hipEvent
pair on the stream (rn_timer_*), after `--warmup` launches of each, min and median over
`--repeats`.

    python tools/fusion_bench.py [--repeats 30] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, V, NEIGHBORS, D, M = 480, 640, 5, 4, 64, 384
GRIDS = [(128, 128, 128), (256, 256, 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fusion_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.appearance import pack_cameras
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.common.scene import get_voxel_grid
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.fusion import _grid_context, fuse_scene
    from raynet_amd.synthetic import make_synthetic_scene
    _lib.build()

    scene, bank = make_synthetic_scene(H=H, W=W, n_views=V, focal=1.5 * H, seed=1234)
    gp = GenerationParameters(depth_planes=D, neighbors=NEIGHBORS,
                              grid_shape=np.array(GRIDS[0], np.int32),
                              max_number_of_marched_voxels=M, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)

    def run_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = [(np.array(m), np.array(s.confidence))
               for m, s in fp.forward_pass(scene, (0, V, 1), with_statistics=True)]
        torch.cuda.synchronize()
        return got, (time.perf_counter() - t0) * 1e3

    run_pass()                                          # warm: contexts, plans, allocations
    pairs, pass_ms = run_pass()
    maps, conf = [m for m, _ in pairs], [c for _, c in pairs]
    bbox = np.asarray(scene.bbox, np.float32).reshape(-1)
    cams = [scene.get_image(i).camera for i in range(V)]

    res = {"tool": "fusion_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "views": V, "H": H, "W": W,
           "forward_pass_with_statistics_ms": round(pass_ms, 2), "grids": {}}
    for grid in GRIDS:
        ctx = _grid_context(bbox, grid)
        dev = ctx.device
        G = ctx.G
        cameras = torch.from_numpy(pack_cameras(cams)).to(dev)
        depths = torch.from_numpy(np.stack(maps)).to(dev).contiguous()
        weights = torch.from_numpy(np.stack(conf)).to(dev).contiguous()
        side = float(((bbox[3:] - bbox[:3]).astype(np.float64) / np.array(grid)).max())
        trunc = 3.0 * side
        tsdf = torch.empty(grid, dtype=torch.float32, device=dev)
        weight = torch.empty(grid, dtype=torch.float32, device=dev)
        # the yardstick's inputs: the voxel centres as points, the depth maps as one-channel images
        points = torch.from_numpy(np.ascontiguousarray(
            get_voxel_grid(bbox, grid).transpose(1, 2, 3, 0).reshape(-1, 3))).to(dev)
        images = depths.reshape(V, H, W, 1)
        colors = torch.empty((G, 1), dtype=torch.float32, device=dev)
        cweight = torch.empty((G,), dtype=torch.float32, device=dev)
        views = torch.empty((G,), dtype=torch.int32, device=dev)
        launches = {
            "tsdf_integrate": lambda: ctx.tsdf_integrate(cameras, depths, None, trunc, 0.0,
                                                         tsdf, weight),
            "tsdf_integrate_weighted": lambda: ctx.tsdf_integrate(cameras, depths, weights, trunc,
                                                                  0.0, tsdf, weight),
            "project_colors": lambda: ctx.project_colors(points, None, cameras, images, depths,
                                                         trunc, 0.0, 0.0, 0, colors, cweight, views),
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
        observed = int((weight > 0).sum().item())
        out = {"G": G, "trunc": round(trunc, 6), "observed_voxels": observed}
        for k in launches:
            med = float(np.median(ms[k]))
            out[k] = {"ms_min": round(float(min(ms[k])), 4), "ms_median": round(med, 4),
                      "point_views_per_s": round(G * V / (med * 1e-3), 1)}
        for k, maps_read in (("tsdf_integrate", 1), ("tsdf_integrate_weighted", 2)):
            must_move = V * H * W * 4 * maps_read + 8 * G
            out[k]["bytes_must_move"] = must_move
            out[k]["GB_per_s"] = round(must_move / (out[k]["ms_median"] * 1e-3) / 1e9, 1)
            out[k]["ratio_to_project_colors"] = round(
                out[k]["ms_median"] / out["project_colors"]["ms_median"], 3)
        # the whole thing, as a user calls it: upload, fuse, iso-surface, cleaning, download
        fuse_scene(scene, maps, range(V), grid, weights=conf).mesh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        volume = fuse_scene(scene, maps, range(V), grid, weights=conf)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mesh = volume.mesh()
        t2 = time.perf_counter()
        out["fuse_scene_ms"] = round((t1 - t0) * 1e3, 2)
        out["mesh_ms"] = round((t2 - t1) * 1e3, 2)
        out["fuse_and_mesh_over_forward_pass"] = round((t2 - t0) * 1e3 / pass_ms, 3)
        out["mesh"] = {"vertices": len(mesh.vertices), "faces": len(mesh.faces)}
        res["grids"]["x".join(str(g) for g in grid)] = out
        del points, colors, cweight, views, tsdf, weight
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
