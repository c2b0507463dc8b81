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
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

H, W, V, NEIGHBORS, D, M = 480, 640, 5, 4, 64, 384
GRID, FUSED_GRID, THRESHOLD = (128, 128, 128), (256, 256, 128), 0.5
MESHES = ("mrf_128", "fused_256")
ITERATIONS, LAMBDA, MU = 10, 0.5, -0.53
STEPS = 2 * ITERATIONS
KERNELS = {"k_smooth_ring": 1, "k_smooth_step": STEPS, "k_vertex_area_normals": 1}   # per turn


def meshes():
    """-> {name: (vertices (nv, 3) f32 device, faces (nf, 3) i32 device)}."""
    import torch
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.fusion import fuse_scene
    from raynet_amd.synthetic import make_synthetic_scene
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=V, focal=1.5 * H, seed=1234)
    gp = GenerationParameters(depth_planes=D, neighbors=NEIGHBORS,
                              grid_shape=np.array(GRID, np.int32),
                              max_number_of_marched_voxels=M, padding=11, gamma_mrf=0.05)
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    pairs = [(np.array(m), np.array(s.confidence))
             for m, s in fp.forward_pass(scene, (0, V, 1), with_statistics=True)]
    out = {}
    mrf = fp.occupancy_volume().mesh(THRESHOLD)
    out["mrf_128"] = (mrf.vertices, mrf.faces)
    fused = fuse_scene(scene, [m for m, _ in pairs], range(V), FUSED_GRID,
                       weights=[c for _, c in pairs]).mesh()
    out["fused_256"] = (fused.vertices, fused.faces)
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda(),
                torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).cuda())
            for k, (v, f) in out.items()}


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


def stats(ms):
    return {"ms_min": round(float(min(ms)), 4), "ms_median": round(float(np.median(ms)), 4)}


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.appearance import corner_table
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.smoothing import boundary_vertices
    _lib.build()
    found = meshes()
    ctx = get_context()
    res = {"tool": "smooth_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "iterations": ITERATIONS, "lambda": LAMBDA, "mu": MU,
           "meshes": {}}
    for name in MESHES:
        vertices, faces = found[name]
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
        if args.trace:
            continue
        step_bytes = 24 * nv + 12 * nv + 24 * nf + 4 * (nv + 1)
        ring_bytes = 12 * nf + 12 * nf + 24 * nf
        entry = {"nv": nv, "nf": nf, "border_vertices": int(border.sum().item()),
                 "bytes_must_move_per_step": step_bytes, "bytes_must_move_ring": ring_bytes}
        for k in launches:
            entry[k] = stats(ms[k])
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
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON."""
    res = json.loads(open(args.out).read())
    turns = res["warmup"] + res["repeats"]
    rows = {k: [] for k in KERNELS}
    with open(args.merge_trace) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for k, per_turn in KERNELS.items():
        rows[k].sort()
        # (the turns are the last dispatches of the run: whatever built the meshes came before)
        expected = per_turn * turns * len(MESHES)
        if len(rows[k]) < expected:
            raise SystemExit("%s: %d dispatches in the trace, expected %d"
                             % (k, len(rows[k]), expected))
        rows[k] = rows[k][-expected:]
    for at, name in enumerate(MESHES):
        own = {}
        for k, per_turn in KERNELS.items():
            mine = rows[k][(at * turns + res["warmup"]) * per_turn:(at + 1) * turns * per_turn]
            own[k] = stats([(e - s) * 1e-6 for s, e in mine])
        entry = res["meshes"][name]
        step, ring = own["k_smooth_step"]["ms_median"], own["k_smooth_ring"]["ms_median"]
        own["k_smooth_step"]["GB_per_s"] = round(
            entry["bytes_must_move_per_step"] / (step * 1e-3) / 1e9, 1)
        own["k_smooth_ring"]["GB_per_s"] = round(
            entry["bytes_must_move_ring"] / (ring * 1e-3) / 1e9, 1)
        own["step_to_normals"] = round(step / own["k_vertex_area_normals"]["ms_median"], 3)
        own["ring_to_step"] = round(ring / step, 3)
        entry["kernel_trace"] = own
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def merge_box(args):
    """bench.py's JSON line of the same visit, under "box"."""
    res = json.loads(open(args.out).read())
    lines = [l for l in open(args.merge_box).read().splitlines() if l.strip().startswith("{")]
    res["box"] = json.loads(lines[-1])
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true",
                    help="only the launches (for a kernel trace); writes nothing")
    ap.add_argument("--merge_trace", default=None,
                    help="a rocprofv3 kernel_trace.csv of --trace: add the kernels' times (no GPU)")
    ap.add_argument("--merge_box", default=None,
                    help="a file with bench.py's JSON line of the same visit (no GPU)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "smooth_bench.json"))
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args)
    elif args.merge_box:
        merge_box(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
