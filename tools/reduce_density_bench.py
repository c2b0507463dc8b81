#!/usr/bin/env python3
"""Timing of the exact parallel density reduction (raynet_amd.metrics.ReduceDensity, DESIGN.md
section 12a) on one GPU: prints one JSON line and writes it to
profiles/reduce_density_bench.json.  The cloud is seeded: five 1280 x 720 wavy depth maps of
ring cameras, back-projected by rn_depthmap_points (about 4.6 M points).  The device part
(keys, sort, gather, rounds; ReduceDensity.keep_mask) is timed from a synchronise to a
synchronise after one warm-up, the median of --repeats; every round ends in the read of its
undecided count, so the rounds are timed one by one as well.  The whole filter() (host checks,
upload, download, the column selection) is timed next to it.

For scale only: the reference's loop restated (scikit-learn's KDTree.query_radius, then the
Python loop) on this machine's CPUs, at the same N if a pilot run on a part of the cloud
predicts less than a minute, otherwise at the pilot's N, which the line states.  No threshold:
this is where the numbers are written down.

    python tools/reduce_density_bench.py [--views 5] [--height 720] [--width 1280]
                                         [--min_distance 0.01] [--seed 0] [--repeats 3]
                                         [--out profiles/reduce_density_bench.json]
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


def make_cloud(views, H, W, seed):
    """(3, views H W) float64 CUDA tensor."""
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.synthetic import ring_cameras
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    clouds = []
    for k, cam in enumerate(ring_cameras(views, H, W, arc=np.pi / 3)):
        depth = (2.6 + 0.2 * np.sin(u * (11.8 / W) + k) * np.cos(v * (11.4 / H)) +
                 0.002 * rng.standard_normal((H, W)))
        pts = torch.empty((3, H * W), dtype=torch.float64, device="cuda")
        get_context().depthmap_points(
            H, W, torch.from_numpy(np.ascontiguousarray(cam.P_pinv, np.float64)).cuda(),
            torch.from_numpy(np.asarray(cam.center, np.float64).reshape(4).copy()).cuda(),
            torch.from_numpy(depth.astype(np.float32)).cuda(), pts)
        clouds.append(pts)
    return torch.cat(clouds, dim=1).contiguous()


def sklearn_loop(X, r, order):
    """Seconds of the reference's loop (raynet/metrics.py:94-127) with an explicit order, and
    the number of points it keeps."""
    from sklearn.neighbors import KDTree
    t0 = time.perf_counter()
    index_set = np.ones(X.shape[1], dtype=bool)
    idx = KDTree(X.T).query_radius(X[:, order].T, r)
    for _id, i in zip(idx, order):
        if index_set[i]:
            index_set[_id] = 0
            index_set[i] = 1
    return time.perf_counter() - t0, int(index_set.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--min_distance", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pilot", type=int, default=200000, help="points of the CPU pilot run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reduce_density_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.metrics import ReduceDensity
    _lib.build()
    pts = make_cloud(args.views, args.height, args.width, args.seed)
    X = pts.cpu().numpy()
    N, r = X.shape[1], args.min_distance
    f = ReduceDensity(r, seed=args.seed)
    lo, h = f._grid(X)
    out = {"tool": "reduce_density_bench", "device": torch.cuda.get_device_name(0), "points": N,
           "views": args.views, "image": [args.height, args.width], "min_distance": r,
           "seed": args.seed}

    keep = f.keep_mask(pts, lo, h)                      # warm-up
    torch.cuda.synchronize()
    runs = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = f.keep_mask(pts, lo, h)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0, list(f.round_seconds)))
    total, rounds = sorted(runs, key=lambda t: t[0])[len(runs) // 2]
    kept = int(keep.sum().item())
    out.update({"kept": kept, "rounds": len(rounds), "device_total_ms": round(1e3 * total, 3),
                "rounds_ms": [round(1e3 * t, 3) for t in rounds],
                "rounds_total_ms": round(1e3 * sum(rounds), 3),
                "keys_sort_gather_ms": round(1e3 * (total - sum(rounds)), 3),
                "mean_round_ms": round(1e3 * sum(rounds) / len(rounds), 3),
                "points_per_s": round(N / total, 1)})
    t0 = time.perf_counter()
    filtered = f.filter(X)
    out["filter_call_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    assert filtered.shape[1] == kept

    cpus = len(os.sched_getaffinity(0))
    try:
        import sklearn
        n_pilot = min(args.pilot, N)
        sub = np.ascontiguousarray(X[:, :n_pilot])
        seconds, kept_cpu = sklearn_loop(sub, r, f.visiting_order(n_pilot))
        row = {"sklearn": sklearn.__version__, "cpus_granted": cpus, "points": n_pilot,
               "seconds": round(seconds, 3), "kept": kept_cpu}
        if n_pilot < N and seconds * N / n_pilot * 1.2 < 60.0:
            seconds, kept_cpu = sklearn_loop(X, r, f.visiting_order(N))
            assert kept_cpu == kept
            row.update({"points": N, "seconds": round(seconds, 3), "kept": kept_cpu})
        elif n_pilot < N:
            row["note"] = ("the same N is predicted to take %.0f s (over a minute): measured on "
                           "the cloud's first %d points" % (seconds * N / n_pilot, n_pilot))
        out["cpu_kd_tree_loop"] = row
    except ImportError:
        out["cpu_kd_tree_loop"] = "scikit-learn is not installed: no CPU line"
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
