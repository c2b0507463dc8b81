#!/usr/bin/env python3
"""What the cross-view check costs: rn_points_consistency against the
rn_consistency_tau launches that cover the same (point, view) pairs.  One process on one GPU; prints
one JSON line and writes it to profiles/consistency_bench.json.

The scene is the synthetic one's geometry at bench.py's image shape: 5 cameras on a ring, 480 x 640,
analytic depth maps of a sphere over a ground plane.  For every view r the 480 x 640 points of its
map (rn_depthmap_points) are checked against the other four views:

    points_consistency   one launch, exclude = r: four views per point, three masks and the
                         residual written once
    consistency_tau x 4  one launch per other view, tau [n] f64 read and written by each

so both columns cover the same 5 x 480 x 640 x 4 pairs; `all_views_one_launch` is one
rn_points_consistency over all 5 x 480 x 640 points with no view excluded (five views per point).
rn_consistency_tau is the library's own, whose kernel this feature does not touch.  The launches
take turns; a hipEvent pair on the stream (rn_timer_*) around `--inner` rounds of one column (a
single round is a tenth of a millisecond, too short a window), after `--warmup` rounds, min and
median of the time per round over `--repeats` windows.  bytes_must_move: the points, the maps and the outputs
once; the rates are these bytes over the median time, not a share of any peak.

    python tools/consistency_bench.py [--repeats 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, V = 480, 640, 5
TOL_ABS, TOL_REL = 0.0, 0.01


def analytic_depth(cam, sphere=((0.0, 0.0, -0.1), 0.5), ground_z=-0.7, ground_radius=0.95):
    """(H, W) float32: the distance from the camera centre to the nearer of a sphere and a ground
    disc along every pixel's ray, 0 where the ray meets neither."""
    K, R = np.asarray(cam.K, np.float64), np.asarray(cam.R, np.float64)
    c = np.asarray(cam.center, np.float64).reshape(-1)[:3]
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([X, Y, np.ones_like(X)], -1) @ np.linalg.inv(K).T @ R
    d /= np.sqrt((d * d).sum(-1, keepdims=True))
    oc = c - np.asarray(sphere[0], np.float64)
    b = d @ oc
    disc = b * b - (oc @ oc - sphere[1] ** 2)
    with np.errstate(all="ignore"):
        t_sphere = np.where(disc >= 0, -b - np.sqrt(disc), np.inf)
        t_ground = (ground_z - c[2]) / d[..., 2]
    t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
    with np.errstate(all="ignore"):
        hit = c + t_ground[..., None] * d
        on_disc = (hit[..., 0] ** 2 + hit[..., 1] ** 2) <= ground_radius ** 2
    t_ground = np.where(np.isfinite(t_ground) & (t_ground > 0) & on_disc, t_ground, np.inf)
    t = np.minimum(t_sphere, t_ground)
    return np.where(np.isfinite(t), t, 0.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=50,
                    help="rounds inside one timed window (a single round is a tenth of a millisecond)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "consistency_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.appearance import pack_cameras
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.synthetic import ring_cameras
    _lib.build()
    if not torch.cuda.is_available():
        raise _lib.RaynetHipError("no GPU visible: a timing needs the MI355X")
    ctx = get_context()
    dev = ctx.device
    cams = ring_cameras(V, H, W, focal=1.5 * H)
    maps = [analytic_depth(c) for c in cams]
    depths = torch.from_numpy(np.stack(maps)).to(dev).contiguous()
    rows = torch.from_numpy(pack_cameras(cams)).to(dev)
    n = H * W
    f64 = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a, np.float64).reshape(shape)).to(dev)  # noqa: E731
    Ps = [f64(c.P, (3, 4)) for c in cams]
    pinvs = [f64(c.P_pinv, (4, 3)) for c in cams]
    centers = [f64(c.center, (4,)) for c in cams]
    points = torch.empty((V, 3, n), dtype=torch.float64, device=dev)
    for r in range(V):
        ctx.depthmap_points(H, W, pinvs[r], centers[r], depths[r], points[r])
    every = points.permute(1, 0, 2).reshape(3, V * n).contiguous()      # [3][V n]
    masks = [torch.empty((V * n,), dtype=torch.int32, device=dev) for _ in range(3)]
    residual = torch.empty((V * n,), dtype=torch.float32, device=dev)
    tau = torch.empty((n,), dtype=torch.float64, device=dev)

    def new():
        for r in range(V):
            ctx.points_consistency(points[r], rows, depths, r, TOL_ABS, TOL_REL, 0.0,
                                   *[m[:n] for m in masks], residual[:n])

    def old():
        for r in range(V):
            for k, v in enumerate(v for v in range(V) if v != r):
                ctx.consistency_tau(H, W, k == 0, points[r], Ps[v], centers[v], depths[v], tau)

    def one():
        ctx.points_consistency(every, rows, depths, -1, TOL_ABS, TOL_REL, 0.0, *masks, residual)

    launches = {"points_consistency": (new, V), "consistency_tau": (old, V * (V - 1)),
                "all_views_one_launch": (one, 1)}
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
    seen = int((masks[0] != 0).sum().item())
    res = {"tool": "consistency_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "inner": args.inner, "views": V, "H": H, "W": W, "points": V * n,
           "tol_abs": TOL_ABS, "tol_rel": TOL_REL, "points_seen_by_a_view": seen}
    pairs = {"points_consistency": V * n * (V - 1), "consistency_tau": V * n * (V - 1),
             "all_views_one_launch": V * n * V}
    must_move = {
        # per view: its points, every other map, four outputs
        "points_consistency": V * (24 * n + (V - 1) * 4 * n + 16 * n),
        # per pair: the points and the map again, tau written (and read but for the first)
        "consistency_tau": V * ((V - 1) * (24 * n + 4 * n + 8 * n) + (V - 2) * 8 * n),
        "all_views_one_launch": 24 * V * n + V * 4 * n + 16 * V * n,
    }
    for k, (_f, count) in launches.items():
        med = float(np.median(ms[k]))
        res[k] = {"launches": count, "ms_min": round(float(min(ms[k])), 4),
                  "ms_median": round(med, 4), "ms_max": round(float(max(ms[k])), 4),
                  "point_views_per_s": round(pairs[k] / (med * 1e-3), 1),
                  "bytes_must_move": must_move[k],
                  "GB_per_s": round(must_move[k] / (med * 1e-3) / 1e9, 1)}
    res["points_consistency"]["ratio_to_consistency_tau"] = round(
        res["points_consistency"]["ms_median"] / res["consistency_tau"]["ms_median"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
