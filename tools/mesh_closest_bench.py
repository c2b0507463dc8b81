#!/usr/bin/env python3
"""Timing of the nearest-surface query (raynet_amd/mesh.py: closest_points) on one GPU: prints
one JSON line and writes it to profiles/mesh_closest_bench.json.  For synthetic box cities
(raynet_amd.synthetic.make_box_city) of 1e5, 1e6 and 4e6 triangles: 1e6 queries -- points of
`sample_surface` plus Gaussian noise of 1 % of the mesh's extent -- through k_mesh_closest,
hipEvent-timed, the median of 3 after one warm-up; the sampler itself likewise.  For the
smallest city, for context, the time of the exact nearest-VERTEX scan (rn_nearest_neighbors,
what metrics.Accuracy runs) over the same queries against the mesh's vertices.  No threshold:
this is where the number is written down.

    python tools/mesh_closest_bench.py [--sizes 100000,1000000,4000000] [--queries 1000000]
                                       [--repeats 3] [--out profiles/mesh_closest_bench.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, repeats):
    """Median milliseconds of fn() over `repeats` hipEvent-timed runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(repeats):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--queries", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mesh_closest_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.mesh import MeshRaycaster
    from raynet_amd.synthetic import make_box_city
    _lib.build()
    nq = args.queries
    sizes = [int(s) for s in args.sizes.split(",")]
    out = {"tool": "mesh_closest_bench", "device": torch.cuda.get_device_name(0),
           "queries": nq, "noise": "1 % of the extent", "meshes": []}
    for n in sizes:
        tri = make_box_city(n, seed=1)
        rc = MeshRaycaster(torch.from_numpy(tri).cuda())
        v = rc.triangles.view(-1, 3)
        ext = float((v.amax(0) - v.amin(0)).max().item())
        ms_sample = timed(lambda: rc.sample_surface(nq, seed=1), args.repeats)
        pts, _ = rc.sample_surface(nq, seed=1)
        g = torch.Generator(device="cuda").manual_seed(1)
        q = (pts.double() + 0.01 * ext * torch.randn((nq, 3), dtype=torch.float64, device="cuda",
                                                     generator=g)).contiguous()
        dist = torch.empty((nq,), dtype=torch.float64, device="cuda")
        closest = torch.empty((nq, 3), dtype=torch.float64, device="cuda")
        idx = torch.empty((nq,), dtype=torch.int32, device="cuda")
        ctx = get_context()
        ms = timed(lambda: ctx.mesh_closest(q, rc.nodes, rc.leaves, dist, closest, idx),
                   args.repeats)
        row = {"triangles": int(len(tri)), "bvh_depth": rc.depth, "extent": round(ext, 4),
               "closest_ms": round(ms, 3), "queries_per_s": round(nq / (ms * 1e-3), 1),
               "sample_ms": round(ms_sample, 3),
               "mean_dist_over_extent": float((dist.mean() / ext).item())}
        if n == min(sizes):
            # context: the exact nearest-vertex scan the vertex-based metrics run
            ref = torch.zeros((v.shape[0], 4), dtype=torch.float32, device="cuda")
            ref[:, :3] = v
            q4 = torch.zeros((nq, 4), dtype=torch.float32, device="cuda")
            q4[:, :3] = q.float()
            d32 = torch.empty((nq,), dtype=torch.float32, device="cuda")
            i32 = torch.empty((nq,), dtype=torch.int32, device="cuda")
            row["nearest_vertex_scan_ms"] = round(
                timed(lambda: ctx.nearest_neighbors(ref, q4, d32, i32), args.repeats), 3)
            row["mean_vertex_dist_over_extent"] = float((d32.double().mean() / ext).item())
        out["meshes"].append(row)
        del rc
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
