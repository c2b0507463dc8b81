#!/usr/bin/env python3
"""What the occupancy volume costs: rn_volume_render against
rn_voxel_traversal -- the same serial DDA per ray; the render adds one gather and the products
per step and writes no list -- and rn_occupancy_grid against the bytes it moves.  One process on
one GPU; prints one JSON line and writes it to profiles/volume_render_bench.json.

The volume is the synthetic scene's after one forward pass at bench.py's shape (5 views of 480 x
640, 64 planes, 128^3 voxels, M = 384); the rays are all 480 x 640 pixels of view 0.  The two
launches take turns; per launch a hipEvent pair on the stream (rn_timer_*), after `--warmup`
launches of each, min and median over `--repeats`.  (The render gathers from the caller's
[gx][gy][gz] array; the 4x4x4-bricked alternative, timed by this tool with
tools/experiments/volume_render_bricked_gather.patch applied, is
profiles/volume_render_bench_layouts.json.)

    python tools/volume_render_bench.py [--repeats 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, V, NEIGHBORS, D, M, GRID = 480, 640, 5, 4, 64, 384, (128, 128, 128)


def timed(ctx, launch):
    ctx.timer_start()
    launch()
    return ctx.timer_stop()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["render"], default=None,
                    help="time the render alone (a counter run of its own)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "volume_render_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.common.scene import get_voxel_grid
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.hip_implementations.context import HipContext
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
    belief = volume.belief
    bbox = scene.bbox.ravel()
    vg = np.ascontiguousarray(get_voxel_grid(bbox, GRID).transpose(1, 2, 3, 0))

    ctx = HipContext(M, 2, 2, 1, H, W, 0, bbox, GRID)
    ctx.set_voxel_grid(vg)
    n = H * W
    cam = scene.get_image(0).camera
    ridx = torch.arange(n, dtype=torch.int32, device="cuda")
    P_inv = ctx.dev(np.ascontiguousarray(cam.P_pinv, dtype=np.float32))
    center = ctx.dev(np.ascontiguousarray(cam.center, dtype=np.float32).ravel()[:3])
    starts = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ends = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    ctx.sample_rays(ridx, P_inv, center, starts, ends)
    rvi = torch.zeros((n, M, 3), dtype=torch.int32, device="cuda")
    rvc = torch.zeros((n,), dtype=torch.int32, device="cuda")
    out = torch.zeros((5, n), dtype=torch.float32, device="cuda")

    launches = {
        "traversal": (ctx, lambda: ctx.voxel_traversal(starts, ends, rvi, rvc)),
        "render": (ctx, lambda: ctx.volume_render(starts, ends, center, belief, out)),
    }
    if args.only:
        launches = {args.only: launches[args.only]}
    for _ in range(args.warmup):
        for c, f in launches.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in launches}
    for _ in range(args.repeats):
        for k, (c, f) in launches.items():
            ms[k].append(timed(c, f))
    torch.cuda.synchronize()
    if args.only:
        print(json.dumps({"only": args.only, "ms_median": float(np.median(ms[args.only]))}))
        return
    steps = int(rvc.to(torch.int64).sum())

    def stat(xs, per=None):
        d = {"ms_min": round(float(min(xs)), 4), "ms_median": round(float(np.median(xs)), 4),
             "ms_max": round(float(max(xs)), 4)}
        if per:
            d["voxel_steps_per_s"] = round(per / (d["ms_median"] * 1e-3), 0)
        return d

    res = {"tool": "volume_render_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup,
           "shape": dict(H=H, W=W, rays=n, grid=GRID, M=M, views=V, D=D),
           "voxel_steps": steps, "mean_steps_per_ray": round(steps / n, 2),
           "rays_without_voxels": int((rvc == 0).sum()),
           "traversal": stat(ms["traversal"], steps)}
    t_med = res["traversal"]["ms_median"]
    res["render"] = stat(ms["render"], steps)
    res["render"]["ratio_to_traversal"] = round(res["render"]["ms_median"] / t_med, 3)

    # rn_occupancy_grid against its bytes: reads the accumulator, writes G floats
    G = GRID[0] * GRID[1] * GRID[2]
    acc_bricks = fp._acc_flat
    acc_grid = fp.accumulator.contiguous()
    fctx = fp._ctx
    bel = torch.empty(GRID, dtype=torch.float32, device="cuda")
    grid_launches = {"from_bricks": lambda: fctx.occupancy_grid(acc_bricks, True, fp._acc_bias, bel),
                     "from_grid": lambda: fctx.occupancy_grid(acc_grid, False, 0.0, bel)}
    gms = {k: [] for k in grid_launches}
    for _ in range(args.warmup):
        for f in grid_launches.values():
            f()
    for _ in range(args.repeats):
        for k, f in grid_launches.items():
            gms[k].append(timed(fctx, f))
    for k, read in (("from_bricks", fctx.acc_size()), ("from_grid", G)):
        d = stat(gms[k])
        d["bytes"] = 4 * (read + G)
        d["GB_per_s"] = round(d["bytes"] / (d["ms_median"] * 1e-3) / 1e9, 1)
        res["occupancy_grid_" + k] = d
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
