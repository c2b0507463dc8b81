#!/usr/bin/env python3
"""Timing of the ground-truth depth from a point cloud (raynet_amd/cloud_depth.py, DESIGN.md
section 14b) on one GPU: prints one JSON line and writes it to profiles/cloud_depth_bench.json.

The cloud is 2e7 surface samples of a 1e5-triangle box city (raynet_amd.synthetic.make_box_city,
MeshRaycaster.sample_surface), the views are 49 ring cameras at 1200 x 1600 that see the whole
city -- the size of a DTU scan.  After one warm-up pass, the median of `--repeats` passes, timed
with hipEvents:

  * zbuffer_ms: rn_cloud_zbuffer for all views into a buffer filled beforehand (fill_ms, the
    torch fill of the buffer, is reported next to it), and point-views per second;
  * landed / skipped: from one pass of the counted entry -- the (point, view) pairs that land on
    a pixel and the share of them whose atomic the pre-test skipped; atomics_per_s follows;
  * filter_ms: the torch hidden-point filter (default parameters) over all views;
  * cloud_read_ms: one plain read of the cloud (a torch sum over it), the floor of any design
    that reads every point once.

    python tools/cloud_depth_bench.py [--points 20000000] [--views 49] [--repeats 3]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _median_ms(fn, repeats, before=None):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(repeats + 1):                    # the first pass is the warm-up
        if before is not None:
            before()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--triangles", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cloud_depth_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.cloud_depth import (EMPTY_BITS, CloudDepthRenderer, camera_rows,
                                        filter_coefficients, hidden_point_filter)
    from raynet_amd.mesh import MeshRaycaster
    from raynet_amd.synthetic import make_box_city, ring_cameras
    _lib.build()
    H, W, V = args.height, args.width, args.views
    rc = MeshRaycaster(make_box_city(args.triangles, seed=1))
    points = rc.sample_surface(args.points, seed=0)[0]
    del rc
    # a ring above the city (10 x 10 x 2.2) that keeps all of it in every image
    cams = ring_cameras(V, H, W, radius=12.0, focal=0.9 * W, heights=[5.0 + 0.05 * v for v in range(V)])
    r = CloudDepthRenderer(points)
    rows_host = camera_rows(cams)
    rows = torch.from_numpy(rows_host).cuda()
    zbuf = torch.empty((V, H, W), dtype=torch.int32, device="cuda")
    ctx = r._ctx

    fill_ms = _median_ms(lambda: zbuf.fill_(EMPTY_BITS), args.repeats)
    zbuffer_ms = _median_ms(lambda: ctx.cloud_zbuffer(r.points, rows, H, W, zbuf), args.repeats,
                            before=lambda: zbuf.fill_(EMPTY_BITS))
    reference = zbuf.clone()
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    zbuf.fill_(EMPTY_BITS)
    ctx.cloud_zbuffer(r.points, rows, H, W, zbuf, counts)
    assert torch.equal(zbuf, reference), "the counted entry gave another buffer"
    del reference
    landed, skipped = (int(c) for c in counts.cpu())
    z0 = zbuf.view(torch.float32)
    filled = int(torch.isfinite(z0).sum().item())
    ks, tf = filter_coefficients(rows_host, 1, 1.5, 1.0)
    kept = [None]

    def run_filter():
        kept[0] = hidden_point_filter(z0, ks, tf, 1) & torch.isfinite(z0)
    filter_ms = _median_ms(run_filter, args.repeats)
    kept_pixels = int(kept[0].sum().item())
    cloud_read_ms = _median_ms(lambda: r.points.sum(), args.repeats)

    atomics = landed - skipped
    out = {"tool": "cloud_depth_bench", "device": torch.cuda.get_device_name(0),
           "points": r.n_points, "views": V, "image": [H, W], "repeats": args.repeats,
           "zbuffer_ms": round(zbuffer_ms, 3), "fill_ms": round(fill_ms, 3),
           "point_views_per_s": round(r.n_points * V / (zbuffer_ms * 1e-3), 1),
           "landed_pairs": landed, "landed_share": round(landed / float(max(r.n_points * V, 1)), 4),
           "skipped_by_pretest": skipped,
           "skipped_share_of_landed": round(skipped / float(max(landed, 1)), 4),
           "atomics": atomics, "atomics_per_s": round(atomics / (zbuffer_ms * 1e-3), 1),
           "filled_pixels": filled, "filled_share": round(filled / float(V * H * W), 4),
           "atomics_per_filled_pixel": round(atomics / float(max(filled, 1)), 3),
           "filter_ms": round(filter_ms, 3), "kept_pixels": kept_pixels,
           "cloud_read_ms": round(cloud_read_ms, 3),
           "cloud_read_gb_per_s": round(r.n_points * 12 / (cloud_read_ms * 1e-3) / 1e9, 1)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
