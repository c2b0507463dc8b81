#!/usr/bin/env python3
"""What the depth statistics cost ("Depth statistics"): the plain depth sweep against
the STATS depth sweep of the same build, in one process on one GPU; prints one JSON line and
writes it to profiles/depth_stats_bench.json.

Two shapes on the synthetic scene bench.py uses (5 views of 480 x 640, all of them reference
images): "config2" -- bench.py's shape, 64 planes, 128^3 voxels, M = 384 (6-chunk bodies) -- and
"cli_defaults" -- the script's defaults, 32 planes, 256 x 256 x 128 voxels, M = 650 (rows of 656:
12-chunk bodies).  Per shape two drivers over one context, one without and one with statistics;
after `--warmup` passes of each:

  * depth_ms: the depth launches of a pass (rn_prof_*: hipEvents around every launch of the
    family), summed per pass, median over `--repeats` passes, the two drivers taking turns;
  * step_ms: a whole pass, launches to maps on the host (eager schedule, no profiling), median
    over `--repeats` passes of one driver after the other.

The plain body is the parent commit's code (profiles/depth_stats_isa_identity.txt), so
depth_ms.plain is also what the sweep cost before.

    python tools/depth_stats_bench.py [--repeats 7] [--warmup 3]
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

SHAPES = {
    "config2": dict(D=64, M=384, grid=(128, 128, 128)),
    "cli_defaults": dict(D=32, M=650, grid=(256, 256, 128)),
}
H, W, V, NEIGHBORS = 480, 640, 5, 4


def measure(name, repeats, warmup):
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.synthetic import make_synthetic_scene
    c = SHAPES[name]
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=V, focal=1.5 * H, seed=1234)
    gp = GenerationParameters(depth_planes=c["D"], neighbors=NEIGHBORS,
                              grid_shape=np.array(c["grid"], np.int32),
                              max_number_of_marched_voxels=c["M"], padding=11, gamma_mrf=0.05)
    cls = get_forward_pass_factory("raynet")
    drivers = {"plain": cls(bank, gp, "sample_in_bbox", (H, W), 0),
               "stats": cls(bank, gp, "sample_in_bbox", (H, W), 0)}

    def run(kind):
        more = dict(with_statistics=True) if kind == "stats" else {}
        for out in drivers[kind].forward_pass(scene, (0, V, 1), **more):
            del out

    for _ in range(warmup):
        for kind in drivers:
            run(kind)
    ctx = drivers["plain"]._ctx
    assert ctx is drivers["stats"]._ctx
    depth_ms = {k: [] for k in drivers}
    launches = {}
    for _ in range(repeats):
        for kind in drivers:
            ctx.prof_begin(only=["depth"])
            run(kind)
            rows = ctx.prof_end()
            torch.cuda.synchronize()
            depth_ms[kind].append(sum(ms for _, _, ms in rows))
            launches[kind] = [(rays, round(ms, 4)) for _, rays, ms in rows]
    step_ms = {}
    for kind in drivers:
        times = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(kind)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        step_ms[kind] = times
    med = lambda xs: float(np.median(xs))
    d_plain, d_stats = med(depth_ms["plain"]), med(depth_ms["stats"])
    s_plain, s_stats = med(step_ms["plain"]), med(step_ms["stats"])
    out = {"shape": dict(c, H=H, W=W, views=V, rows_M=drivers["plain"]._rows_M()),
           "captured": bool(drivers["plain"].captured or drivers["stats"].captured),
           "depth_ms": {"plain": round(d_plain, 4), "stats": round(d_stats, 4),
                        "overhead": round(d_stats / d_plain - 1, 4),
                        "spread_plain": [round(min(depth_ms["plain"]), 4), round(max(depth_ms["plain"]), 4)],
                        "spread_stats": [round(min(depth_ms["stats"]), 4), round(max(depth_ms["stats"]), 4)]},
           "last_pass_launches": launches,
           "step_ms": {"plain": round(s_plain, 3), "stats": round(s_stats, 3),
                       "extra": round(s_stats - s_plain, 3),
                       "spread_plain": [round(min(step_ms["plain"]), 3), round(max(step_ms["plain"]), 3)],
                       "spread_stats": [round(min(step_ms["stats"]), 3), round(max(step_ms["stats"]), 3)]}}
    del drivers
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="config2,cli_defaults")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_stats_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    _lib.build()
    out = {"tool": "depth_stats_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup}
    for name in args.shapes.split(","):
        out[name] = measure(name, args.repeats, args.warmup)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
