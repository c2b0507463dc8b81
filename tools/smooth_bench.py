#!/usr/bin/env python3
"""What Taubin smoothing of a mesh costs: rn_mesh_smooth with 10 iterations
-- one ring launch and 20 steps -- on two meshes, against rn_vertex_area_normals on the same mesh
(one gather over the same corner table), the launches taking turns.

  mrf_128       the MRF's surface of the synthetic scene after a pass at bench.py's shape (128^3)
  fused_256     the mesh fused from that pass's depth maps at 256 x 256 x 128 (fusion_bench's)

One process on one GPU.  Per call of the entry a hipEvent pair on the stream (rn_timer_*), after
`--warmup` calls, min and median over `--repeats`.  "Must move" per step is 24 nv (a row read and a
row written) + 12 nv (the clamp's originals) + 24 nf (the ring) + 4 (nv + 1) (the offsets) bytes;
the ring's build moves 12 nf + 12 nf + 24 nf (corners, faces, ring).  The host figure is ten
iterations of the same scheme by np.add.at on mrf_128 (float64 sums, float32 positions between the
steps; not the truth's loop, which is too slow to mean anything).  Prints one JSON line and writes
it to profiles/smooth_bench.json.

The ring launch and one step cannot be bracketed from outside the entry, so they come out of a
kernel trace of their own, with the normals launch beside them:

    python tools/smooth_bench.py [--repeats 30] [--warmup 5]
    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/smooth_bench.py --trace
    python tools/smooth_bench.py --merge_trace DIR/.../*_kernel_trace.csv
    python tools/smooth_bench.py --merge_box FILE      # bench.py's JSON line of the same visit

--trace runs nothing but the meshes' warm-ups and repeats; --merge_trace and --merge_box (no GPU)
add the kernels' own times per mesh, the two ratios of section 23, and the box's speed to the JSON.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_bench as mb  # noqa: E402  (puts the repository on the path)

import numpy as np  # noqa: E402

MESHES = mb.MESHES
ITERATIONS, LAMBDA, MU = 10, 0.5, -0.53
STEPS = 2 * ITERATIONS
KERNELS = {"k_smooth_ring": 1, "k_smooth_step": STEPS, "k_vertex_area_normals": 1}   # per turn


def host_smooth(vertices, faces, fixed):
    """Ten iterations by np.add.at on the host -> (seconds, the positions)."""
    f = faces.astype(np.int64)
    mine = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    a = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 2], f[:, 0], f[:, 1]])
    m = 2.0 * np.bincount(mine, minlength=len(vertices))
    stay = (m == 0) | fixed
    now = vertices.copy()
    t0 = time.perf_counter()
    for _ in range(ITERATIONS):
        for t in (LAMBDA, MU):
            p = now.astype(np.float64)
            s = np.zeros_like(p)
            np.add.at(s, mine, p[a])
            np.add.at(s, mine, p[b])
            x = p + t * (s / np.where(stay, 1.0, m)[:, None] - p)
            now = np.where(stay[:, None], now, x.astype(np.float32))
    return time.perf_counter() - t0, now


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.appearance import corner_table
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.smoothing import boundary_vertices
    _lib.build()
    found = mb.bench_meshes()
    ctx = get_context()
    res = {"tool": "smooth_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "iterations": ITERATIONS, "lambda": LAMBDA, "mu": MU,
           "meshes": {}}
    for name in MESHES:
        vertices, faces, _ = found[name]
        nv, nf = len(vertices), len(faces)
        offsets, corners = corner_table(faces, nv)
        border = boundary_vertices(faces, nv)
        fixed = border.to(torch.uint8)
        work = torch.empty((ctx.mesh_smooth_workspace_bytes(nv, nf),), dtype=torch.uint8,
                           device="cuda")
        out = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        normals = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        launches = {
            "smooth": lambda: ctx.mesh_smooth(vertices, faces, offsets, corners, fixed, ITERATIONS,
                                              LAMBDA, MU, float("inf"), work, out),
            "normals_alone": lambda: ctx.vertex_area_normals(vertices, faces, offsets, corners,
                                                             normals),
        }
        ms = mb.take_turns(ctx, launches, args.warmup, args.repeats)
        if args.trace:
            continue
        step_bytes = 24 * nv + 12 * nv + 24 * nf + 4 * (nv + 1)
        ring_bytes = 12 * nf + 12 * nf + 24 * nf
        entry = {"nv": nv, "nf": nf, "border_vertices": int(border.sum().item()),
                 "bytes_must_move_per_step": step_bytes, "bytes_must_move_ring": ring_bytes}
        for k in launches:
            entry[k] = mb.stats(ms[k])
        entry["smooth"]["GB_per_s"] = round(
            (STEPS * step_bytes + ring_bytes) / (entry["smooth"]["ms_median"] * 1e-3) / 1e9, 1)
        entry["smooth"]["ratio_to_normals_alone"] = round(
            entry["smooth"]["ms_median"] / entry["normals_alone"]["ms_median"], 3)
        moved = (out - vertices).abs()
        entry["farthest_move"] = round(float(moved[torch.isfinite(moved)].max().item()), 6)
        if name == "mrf_128":
            seconds, host = host_smooth(vertices.cpu().numpy(), faces.cpu().numpy(),
                                        border.cpu().numpy())
            entry["host"] = {"what": "np.add.at, %d iterations" % ITERATIONS,
                             "ms": round(seconds * 1e3, 1),
                             "largest_difference_from_the_gpu": float(
                                 np.nanmax(np.abs(host - out.cpu().numpy())))}
        res["meshes"][name] = entry
    if args.trace:
        return
    mb.write_record(res, args.out)


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON."""
    res = json.loads(open(args.out).read())
    turns = res["warmup"] + res["repeats"]
    rows = mb.keep_last(mb.trace_rows(args.merge_trace, KERNELS),
                        {k: per_turn * turns * len(MESHES) for k, per_turn in KERNELS.items()})
    for at, name in enumerate(MESHES):
        own = {}
        for k, per_turn in KERNELS.items():
            mine = rows[k][(at * turns + res["warmup"]) * per_turn:(at + 1) * turns * per_turn]
            own[k] = mb.stats([(e - s) * 1e-6 for s, e in mine])
        entry = res["meshes"][name]
        step, ring = own["k_smooth_step"]["ms_median"], own["k_smooth_ring"]["ms_median"]
        own["k_smooth_step"]["GB_per_s"] = round(
            entry["bytes_must_move_per_step"] / (step * 1e-3) / 1e9, 1)
        own["k_smooth_ring"]["GB_per_s"] = round(
            entry["bytes_must_move_ring"] / (ring * 1e-3) / 1e9, 1)
        own["step_to_normals"] = round(step / own["k_vertex_area_normals"]["ms_median"], 3)
        own["ring_to_step"] = round(ring / step, 3)
        entry["kernel_trace"] = own
    mb.write_record(res, args.out)


if __name__ == "__main__":
    mb.main("smooth_bench", measure, merge_trace)
