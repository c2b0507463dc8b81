#!/usr/bin/env python3
"""What capping the small holes of a mesh costs: rn_mesh_fill_holes with
max_edges of 16, 64 and 1024 on two meshes, against `appearance.corner_table`, which the entry needs
first, and against rn_mesh_components on the same mesh (the chain's other union-find), the three
taking turns.

  mrf_128       the MRF's surface of the synthetic scene after a pass at bench.py's shape (128^3)
  fused_256     the mesh fused from that pass's depth maps at 256 x 256 x 128 (fusion_bench's)

One process on one GPU.  Per call a hipEvent pair on the stream (rn_timer_*), after `--warmup`
calls, min and median over `--repeats`.  The entry waits for the stream once (its status word), so
the pair brackets that wait too.  Recorded per mesh: how many loops it has and how long they are;
per max_edges: how many are filled and how many faces that adds.

Also, recorded and not asserted: surface_completeness of the two-sphere chain of
tests/test_holes_gpu.py (a patch of depth pixels blanked in every view) with `--fill_holes 40` and
without it, against the large sphere as the ground-truth mesh.  Prints one JSON line and writes it
to profiles/holes_bench.json.

The kernels cannot be bracketed from outside the entry, so they come out of a kernel trace of
their own:

    python tools/holes_bench.py [--repeats 30] [--warmup 5]
    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/holes_bench.py --trace
    python tools/holes_bench.py --merge_trace DIR/.../*_kernel_trace.csv
    python tools/holes_bench.py --merge_box FILE      # bench.py's JSON line of the same visit

--trace runs nothing but the warm-ups and repeats of the entry; --merge_trace and --merge_box (no
GPU) add the kernels' own times and the box's speed to the JSON.
"""
import argparse
import csv
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tools"))
from simplify_bench import meshes, stats  # noqa: E402  (the two meshes of sections 23 and 24)

MESHES = ("mrf_128", "fused_256")
MAX_EDGES = (16, 64, 1024)
OWN = ("k_holes_init", "k_holes_edges", "k_holes_flatten", "k_holes_tally", "k_holes_flags",
       "k_holes_emit")


def loop_lengths(ctx, vertices, faces, offsets, corners):
    """The lengths of the simple loops, ascending, and the number of loops that are not simple:
    the entry once with every length allowed; a filled loop's length is its number of new faces."""
    import torch
    new_vertices, new_faces, source, counts = ctx.mesh_fill_holes(vertices, faces, offsets, corners, 65536)
    centre = new_faces[:, 2].to(torch.int64) - len(vertices)
    lengths = torch.bincount(centre, minlength=len(source)).cpu().numpy()
    return np.sort(lengths), counts


def two_sphere_chain():
    """surface_completeness of the two-sphere chain with the stage and without it."""
    import torch  # noqa: F401
    from PIL import Image as PILImage
    from raynet_amd.common.scene import get_scene
    from raynet_amd.metrics import SurfaceCompleteness
    from raynet_amd.scripts import fuse_depth_maps
    from raynet_amd.synthetic import ring_cameras
    from raynet_amd.volume import SurfaceMesh
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import fusion_truth as ft
    F, H, W, grid = np.float32, 20, 30, (18, 22, 14)
    big, small = ((0.0, 0.0, -0.1), 0.5), ((-0.6, 0.55, 0.5), 0.15)
    cams = ring_cameras(3, H, W, focal=1.5 * H)
    rng = np.random.default_rng(0)
    out = {"patch": "rows 9:11, columns 14:16 of every view", "max_edges": 40, "samples": 2000}
    with tempfile.TemporaryDirectory() as tmp:
        scene_dir, preds = os.path.join(tmp, "scene"), os.path.join(tmp, "predictions")
        for d in ("imgs", "cams_krt", "gt"):
            os.makedirs(os.path.join(scene_dir, d))
        os.makedirs(preds)
        with open(os.path.join(scene_dir, "scene_info.xml"), "w") as f:
            f.write('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<bwm_info_for_boxm2>\n'
                    '  <bbox minx="-1" miny="-1" minz="-1" maxx="1" maxy="1" maxz="1">\n'
                    '  </bbox>\n</bwm_info_for_boxm2>\n')
        for i, cam in enumerate(cams):
            d = np.minimum(ft.sphere_depth(cam, H, W, *big), ft.sphere_depth(cam, H, W, *small))
            d = np.where(np.isfinite(d), d, F(0)).astype(F)
            d = np.where(d > 0, d + rng.normal(scale=0.02, size=d.shape).astype(F), F(0)).astype(F)
            d[9:11, 14:16] = 0
            np.save(os.path.join(scene_dir, "gt", "gt_depth_%d.npy" % i), d)
            PILImage.fromarray(np.full((H, W, 3), 40 * i + 60, np.uint8)).save(
                os.path.join(scene_dir, "imgs", "frame_%03d.png" % i))
            with open(os.path.join(scene_dir, "cams_krt", "frame_%03d.txt" % i), "w") as f:
                for row in np.asarray(cam.K, np.float64):
                    f.write(" ".join("%.9g" % x for x in row) + "\n")
                f.write("\n")
                for row in np.asarray(cam.R, np.float64):
                    f.write(" ".join("%.9g" % x for x in row) + "\n")
                f.write("\n" + " ".join("%.9g" % x for x in np.asarray(cam.t, np.float64).ravel()) + "\n")
        # the ground truth: the large sphere as a latitude-longitude mesh
        n_lat, n_lon = 48, 96
        lat = np.pi * (np.arange(n_lat + 1) / n_lat)
        lon = 2.0 * np.pi * np.arange(n_lon) / n_lon
        p = np.stack([np.outer(np.sin(lat), np.cos(lon)), np.outer(np.sin(lat), np.sin(lon)),
                      np.outer(np.cos(lat), np.ones(n_lon))], -1).reshape(-1, 3)
        p = (np.array(big[0]) + big[1] * p).astype(F)
        i, j = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
        q, r = (i * n_lon + j).reshape(-1), (i * n_lon + (j + 1) % n_lon).reshape(-1)
        faces = np.concatenate([np.stack([q, q + n_lon, r + n_lon], 1), np.stack([q, r + n_lon, r], 1)])
        SurfaceMesh(p, faces.astype(np.int32)).save_ply(os.path.join(scene_dir, "gt_mesh.ply"))
        scene = get_scene("restrepo", scene_dir)
        common = ["--gt", "--truncation", "0.25", "--start_end", "0,3", "--grid_shape", "18,22,14",
                  "--keep_largest", "1", "--smooth", "5", "--normals"]
        side = float((2.0 / np.array(grid, np.float64)).min())
        for name, flags in (("without", []), ("with", ["--fill_holes", "40"])):
            ply = os.path.join(tmp, name + ".ply")
            fuse_depth_maps.main([scene_dir, preds, ply] + flags + common)
            mesh = SurfaceMesh.load_ply(ply)
            dist, _ = SurfaceCompleteness(2000, seed=0).compute(scene, [0, 1, 2], None,
                                                                mesh.pointcloud(20000, 3))
            dist = np.asarray(dist, np.float64).reshape(-1)
            out[name] = {"faces": len(mesh.faces), "mean": round(float(dist.mean()), 5),
                         "median": round(float(np.median(dist)), 5),
                         "share_within_one_voxel_side": round(float((dist <= side).mean()), 4)}
    return out


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.appearance import corner_table
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.hip_implementations.context import _ptr, _stream
    _lib.build()
    found = meshes()
    ctx = get_context()
    res = {"tool": "holes_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "max_edges": list(MAX_EDGES), "meshes": {}}
    for name in MESHES:
        vertices, faces, _ = found[name]
        nv, nf = len(vertices), len(faces)
        offsets, corners = corner_table(faces, nv)
        labels, vc, fc = (torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(3))
        status = torch.zeros((1,), dtype=torch.int32, device="cuda")
        nvo = torch.empty((nf, 3), dtype=torch.float32, device="cuda")
        nfo = torch.empty((3 * nf, 3), dtype=torch.int32, device="cuda")
        so = torch.empty((nf,), dtype=torch.int32, device="cuda")
        counts = torch.zeros((5,), dtype=torch.int64, device="cuda")
        work = torch.empty((ctx.mesh_fill_holes_workspace_bytes(nv, nf),), dtype=torch.uint8,
                           device="cuda")
        entry = {"nv": nv, "nf": nf, "workspace_bytes": int(work.numel()), "max_edges": {}}
        if not args.trace:
            lengths, all_counts = loop_lengths(ctx, vertices, faces, offsets, corners)
            entry.update(loops=int(all_counts[2]), loops_not_simple=int(all_counts[3]),
                         boundary_half_edges=int(all_counts[4]),
                         simple_loop_lengths={"count": len(lengths),
                                              "median": int(np.median(lengths)) if len(lengths) else 0,
                                              "longest": int(lengths[-1]) if len(lengths) else 0,
                                              "up_to_16": int((lengths <= 16).sum()),
                                              "up_to_64": int((lengths <= 64).sum()),
                                              "up_to_1024": int((lengths <= 1024).sum())})
        for max_edges in MAX_EDGES:
            launches = {
                "fill_holes": lambda: ctx._check(ctx.lib.rn_mesh_fill_holes(
                    ctx._h, nv, _ptr(vertices), nf, _ptr(faces), _ptr(offsets), _ptr(corners),
                    max_edges, _ptr(nvo), _ptr(nfo), _ptr(so), _ptr(counts), _ptr(work), _stream())),
                "corner_table": lambda: corner_table(faces, nv),
                "components": lambda: ctx._check(ctx.lib.rn_mesh_components(
                    ctx._h, nv, nf, _ptr(faces), _ptr(labels), _ptr(vc), _ptr(fc), _ptr(status),
                    _stream())),
            }
            if args.trace:
                launches = {"fill_holes": launches["fill_holes"]}
            ms = {k: [] for k in launches}
            for i in range(args.warmup + args.repeats):
                for k, f in launches.items():
                    ctx.timer_start()
                    f()
                    ms[k].append(ctx.timer_stop())
            torch.cuda.synchronize()
            if args.trace:
                continue
            got = counts.tolist()
            one = {"filled": got[0], "new_faces": got[1],
                   "longest_filled": int(lengths[lengths <= max_edges][-1]) if (lengths <= max_edges).any() else 0}
            for k in launches:
                one[k] = stats(ms[k][args.warmup:])
            one["fill_holes"]["ratio_to_components"] = round(
                one["fill_holes"]["ms_median"] / one["components"]["ms_median"], 3)
            entry["max_edges"]["%d" % max_edges] = one
        res["meshes"][name] = entry
    if args.trace:
        return
    res["two_sphere_chain_surface_completeness"] = two_sphere_chain()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON: every
    kernel of the entry is dispatched once per call, so the calls are the last dispatches of the
    run, in the order of the meshes and of max_edges."""
    res = json.loads(open(args.out).read())
    turns = res["warmup"] + res["repeats"]
    rows = {k: [] for k in OWN}
    with open(args.merge_trace) as f:
        for row in csv.DictReader(f):
            for k in OWN:
                if k in row["Kernel_Name"]:
                    rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    plan = [(name, "%d" % m) for name in MESHES for m in res["max_edges"]]
    for k in OWN:
        rows[k].sort()
        if len(rows[k]) < len(plan) * turns:
            raise SystemExit("%s: %d dispatches in the trace, expected %d"
                             % (k, len(rows[k]), len(plan) * turns))
        rows[k] = rows[k][-len(plan) * turns:]
    for at, (name, m) in enumerate(plan):
        own = {}
        for k in OWN:
            mine = rows[k][at * turns:(at + 1) * turns][res["warmup"]:]
            own[k] = stats([(e - s) * 1e-6 for s, e in mine])
        own["sum_of_own_kernels_ms"] = round(sum(own[k]["ms_median"] for k in OWN), 4)
        res["meshes"][name]["max_edges"][m]["kernel_trace"] = own
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
                    help="only the entry's launches (for a kernel trace); writes nothing")
    ap.add_argument("--merge_trace", default=None,
                    help="a rocprofv3 kernel_trace.csv of --trace: add the kernels' times (no GPU)")
    ap.add_argument("--merge_box", default=None,
                    help="a file with bench.py's JSON line of the same visit (no GPU)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "holes_bench.json"))
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args)
    elif args.merge_box:
        merge_box(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
