#!/usr/bin/env python3
"""What choosing views costs: rn_view_overlap at 5 and 49 views over a
million points, with and without depth maps, rn_points_consistency on the same points and views
(up to its limit of 32) as the yardstick of phase one, and eight rounds of rn_view_gain.  One
process on one GPU; prints one JSON line and writes it to profiles/view_selection_bench.json.

The scene: V cameras on a ring (the synthetic scene's, at 480 x 640) around the box [-1, 1]^3,
analytic depth maps of a sphere over a ground disc (tools/consistency_bench.py's), and 2^20 points
drawn uniformly from the box -- a proxy grid's worth, most of them seen by most views, which is the
expensive case for the pair phase.  Columns, per V in (5, 49):

    view_overlap            rn_view_overlap, no normals, no depth maps (a proxy grid)
    view_overlap_depths     ... with the V depth maps as occluders
    points_consistency      rn_points_consistency on the same points, min(V, 32) views and their
                            maps, no view excluded: projection and one gather per view, four
                            outputs -- what phase one of rn_view_overlap does, without the pairs
    view_gain_x8            eight rn_view_gain launches over the masks (a covering set of eight),
                            without the read-backs between them

The columns take turns; a hipEvent pair on the stream (rn_timer_*) around `--inner` rounds of one
column, after `--warmup` rounds, min and median of the time per round over `--repeats` windows.
pair_tests: the (point, pair of views) combinations both of whose views see the point -- the pair
tests the kernel runs per lane are at least these (a wavefront runs a pair for all its lanes when
any lane needs it).  No ratio is promised; the figures are what was measured.

    python tools/view_selection_bench.py [--repeats 20] [--warmup 3] [--inner 5]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 480, 640
N = 1 << 20
VIEWS = (5, 49)
ROUNDS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="rounds inside one timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "view_selection_bench.json"))
    args = ap.parse_args()
    from consistency_bench import analytic_depth
    from raynet_amd import _lib
    from raynet_amd.appearance import pack_cameras
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.synthetic import ring_cameras
    from raynet_amd.view_selection import band_cosines
    _lib.build()
    if not torch.cuda.is_available():
        raise _lib.RaynetHipError("no GPU visible: a timing needs the MI355X")
    ctx = get_context()
    dev = ctx.device
    rng = np.random.default_rng(0)
    points = torch.from_numpy(rng.uniform(-1.0, 1.0, (3, N))).to(dev).contiguous()
    cos_lo, cos_hi = band_cosines(2.0, 45.0)
    visible = torch.empty((N,), dtype=torch.int64, device=dev)
    masks = [torch.empty((N,), dtype=torch.int32, device=dev) for _ in range(3)]
    residual = torch.empty((N,), dtype=torch.float32, device=dev)
    res = {"tool": "view_selection_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "inner": args.inner, "points": N, "H": H, "W": W,
           "min_angle": 2.0, "max_angle": 45.0, "gain_rounds": ROUNDS}
    for V in VIEWS:
        cams = ring_cameras(V, H, W, focal=1.5 * H,
                            heights=[0.3 + 0.2 * (v % 5) for v in range(V)])
        rows = torch.from_numpy(pack_cameras(cams)).to(dev)
        depths = torch.from_numpy(np.stack([analytic_depth(c) for c in cams])).to(dev).contiguous()
        pairs = torch.zeros((V, V), dtype=torch.int64, device=dev)
        gain = torch.zeros((V + 1,), dtype=torch.int64, device=dev)
        Vc = min(V, 32)

        def plain():
            ctx.view_overlap(points, None, rows, (H, W), None, 0.0, 0.0, 0.0, cos_lo, cos_hi,
                             visible, pairs)

        def occluded():
            ctx.view_overlap(points, None, rows, (H, W), depths, 0.05, 0.0, 0.0, cos_lo, cos_hi,
                             visible, pairs)

        def yardstick():
            ctx.points_consistency(points, rows[:Vc], depths[:Vc], -1, 0.05, 0.0, 0.0, *masks,
                                   residual)

        def gains():
            chosen = 0
            for r in range(ROUNDS):
                ctx.view_gain(visible, V, chosen, 1, gain)
                chosen |= 1 << ((r * 7) % V)

        # what the pair phase has to do, from the masks of the two flavours
        stats = {}
        for name, f in (("view_overlap", plain), ("view_overlap_depths", occluded)):
            pairs.zero_()
            f()
            torch.cuda.synchronize()
            m = visible.cpu().numpy().view(np.uint64)
            k = np.unpackbits(m.view(np.uint8).reshape(-1, 8), axis=1).sum(1, dtype=np.int64)
            upper = pairs.cpu().numpy()
            stats[name] = {"seen_point_views": int(k.sum()),
                           "pair_tests": int((k * (k - 1) // 2).sum()),
                           "shared_point_pairs": int(np.triu(upper, 1).sum())}
        plain()                                 # the masks view_gain reads: the denser flavour
        launches = {"view_overlap": (plain, 1), "view_overlap_depths": (occluded, 1),
                    "points_consistency": (yardstick, 1), "view_gain_x8": (gains, ROUNDS)}
        for _ in range(args.warmup):
            for f, _count in launches.values():
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in launches}
        for _ in range(args.repeats):
            for k, (f, _count) in launches.items():
                ctx.timer_start()
                for _ in range(args.inner):
                    f()
                ms[k].append(ctx.timer_stop() / args.inner)
        torch.cuda.synchronize()
        out = {"views": V, "yardstick_views": Vc}
        for k, (_f, count) in launches.items():
            med = float(np.median(ms[k]))
            out[k] = {"launches": count, "ms_min": round(float(min(ms[k])), 4),
                      "ms_median": round(med, 4), "ms_max": round(float(max(ms[k])), 4)}
            if k in stats:
                out[k].update(stats[k])
                out[k]["point_views_per_s"] = round(N * V / (med * 1e-3), 1)
                out[k]["pair_tests_per_s"] = round(stats[k]["pair_tests"] / (med * 1e-3), 1)
            elif k == "points_consistency":
                out[k]["point_views_per_s"] = round(N * Vc / (med * 1e-3), 1)
            else:
                out[k]["ms_per_launch"] = round(med / count, 4)
                out[k]["GB_per_s_of_masks"] = round(count * 8 * N / (med * 1e-3) / 1e9, 1)
        res["V%d" % V] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
