#!/usr/bin/env python3
"""What the surface extraction costs: rn_isosurface_count (classify and
the grid-level scan, with its read-back of the totals) and rn_isosurface_emit, each against the
bytes it has to move, at the bandwidth rn_occupancy_grid -- one streaming pass over the same
volume, the yardstick -- reaches in the same process.  One process on one GPU; prints one JSON
line and writes it to profiles/isosurface_bench.json.

The volume is the synthetic scene's after one forward pass at bench.py's shape (5 views of 480 x
640, 64 planes, 128^3 voxels, M = 384); the surface is taken closed at threshold 0.5 (a 130^3
lattice).  The three launches take turns; per launch a hipEvent pair on the stream (rn_timer_*),
after `--warmup` launches of each, min and median over `--repeats`.

    python tools/isosurface_bench.py [--repeats 30] [--warmup 5] [--only count|emit]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, V, NEIGHBORS, D, M, GRID = 480, 640, 5, 4, 64, 384, (128, 128, 128)
THRESHOLD, CLOSED = 0.5, 1
SCAN_TILE = 256


def scan_words(n):
    """64-bit words the scan reads and writes for n entries: a read per level for the sums, a
    read and a write per level for the scan itself."""
    words = 0
    while n > SCAN_TILE:
        words += 3 * n
        n = (n + SCAN_TILE - 1) // SCAN_TILE
    return words + 2 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["count", "emit"], default=None,
                    help="time one entry alone (a counter run of its own)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "isosurface_bench.json"))
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.hip_implementations.context import _ptr, _stream
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
    ctx = volume._context((1, 1), None)
    lib, h = ctx.lib, ctx._h

    G = GRID[0] * GRID[1] * GRID[2]
    L = (GRID[0] + 2 * CLOSED) * (GRID[1] + 2 * CLOSED) * (GRID[2] + 2 * CLOSED)
    work = torch.empty((lib.rn_isosurface_workspace_bytes(h, CLOSED),), dtype=torch.uint8,
                       device="cuda")
    totals = (ctypes.c_int64 * 2)()

    def count():
        ctx._check(lib.rn_isosurface_count(h, _ptr(belief), THRESHOLD, CLOSED, _ptr(work), totals,
                                           _stream()))

    count()
    nv, nf = int(totals[0]), int(totals[1])
    vertices = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    faces = torch.empty((nf, 3), dtype=torch.int32, device="cuda")

    def emit():
        ctx._check(lib.rn_isosurface_emit(h, _ptr(belief), THRESHOLD, CLOSED, _ptr(work), nv, nf,
                                          _ptr(vertices), _ptr(faces), _stream()))

    acc_grid = fp.accumulator.contiguous()
    bel = torch.empty(GRID, dtype=torch.float32, device="cuda")
    launches = {"occupancy_grid": lambda: fp._ctx.occupancy_grid(acc_grid, False, 0.0, bel),
                "count": count, "emit": emit}
    if args.only:
        launches = {args.only: launches[args.only]}
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
    if args.only:
        print(json.dumps({"only": args.only, "ms_median": float(np.median(ms[args.only]))}))
        return

    # the bytes every pass has to move once: volume, workspace, outputs
    bytes_ = {
        "occupancy_grid": {"volume_read": 4 * G, "volume_written": 4 * G},
        "count": {"volume": 4 * G, "workspace_classify": 9 * L, "workspace_scan": 8 * scan_words(L)},
        "emit": {"volume": 4 * G, "workspace": 9 * L, "outputs": 12 * nv + 12 * nf},
    }
    res = {"tool": "isosurface_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup,
           "shape": dict(grid=GRID, closed=CLOSED, threshold=THRESHOLD, lattice_points=L,
                         views=V, H=H, W=W, D=D, M=M),
           "nv": nv, "nf": nf, "occupied_voxels": int((belief >= THRESHOLD).sum())}
    for k in launches:
        total = sum(bytes_[k].values())
        med = float(np.median(ms[k]))
        res[k] = {"ms_min": round(float(min(ms[k])), 4), "ms_median": round(med, 4),
                  "ms_max": round(float(max(ms[k])), 4), "bytes": dict(bytes_[k], total=total),
                  "GB_per_s": round(total / (med * 1e-3) / 1e9, 1)}
    yard = res["occupancy_grid"]["GB_per_s"] * 1e9
    for k in ("count", "emit"):
        at_yardstick = res[k]["bytes"]["total"] / yard * 1e3
        res[k]["ms_at_yardstick_bandwidth"] = round(at_yardstick, 4)
        res[k]["ratio_to_that"] = round(res[k]["ms_median"] / at_yardstick, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
