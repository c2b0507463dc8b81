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
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_bench as mb  # noqa: E402  (puts the repository on the path)

import numpy as np  # noqa: E402

MESHES = mb.MESHES
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
    from raynet_amd.common.scene import get_scene
    from raynet_amd.metrics import SurfaceCompleteness
    from raynet_amd.scripts import fuse_depth_maps
    from raynet_amd.volume import SurfaceMesh
    sys.path.insert(0, os.path.join(mb.REPO, "tests"))
    import mesh_harness as h
    F = np.float32
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED,
                                                                    blank=h.PATCH)
    out = {"patch": "rows 9:11, columns 14:16 of every view", "max_edges": 40, "samples": 2000}
    with tempfile.TemporaryDirectory() as tmp:
        scene_dir, preds = os.path.join(tmp, "scene"), os.path.join(tmp, "predictions")
        h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
        os.makedirs(preds)
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
    found = mb.bench_meshes()
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
            ms = mb.take_turns(ctx, launches, args.warmup, args.repeats)
            if args.trace:
                continue
            got = counts.tolist()
            one = {"filled": got[0], "new_faces": got[1],
                   "longest_filled": int(lengths[lengths <= max_edges][-1]) if (lengths <= max_edges).any() else 0}
            for k in launches:
                one[k] = mb.stats(ms[k])
            one["fill_holes"]["ratio_to_components"] = round(
                one["fill_holes"]["ms_median"] / one["components"]["ms_median"], 3)
            entry["max_edges"]["%d" % max_edges] = one
        res["meshes"][name] = entry
    if args.trace:
        return
    res["two_sphere_chain_surface_completeness"] = two_sphere_chain()
    mb.write_record(res, args.out)


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON: every
    kernel of the entry is dispatched once per call, so the calls are the last dispatches of the
    run, in the order of the meshes and of max_edges."""
    res = json.loads(open(args.out).read())
    turns = res["warmup"] + res["repeats"]
    plan = [(name, "%d" % m) for name in MESHES for m in res["max_edges"]]
    rows = mb.keep_last(mb.trace_rows(args.merge_trace, OWN), {k: len(plan) * turns for k in OWN})
    for at, (name, m) in enumerate(plan):
        own = {}
        for k in OWN:
            mine = rows[k][at * turns:(at + 1) * turns][res["warmup"]:]
            own[k] = mb.stats([(e - s) * 1e-6 for s, e in mine])
        own["sum_of_own_kernels_ms"] = round(sum(own[k]["ms_median"] for k in OWN), 4)
        res["meshes"][name]["max_edges"][m]["kernel_trace"] = own
    mb.write_record(res, args.out)


if __name__ == "__main__":
    mb.main("holes_bench", measure, merge_trace)
