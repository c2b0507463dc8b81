#!/usr/bin/env python3
"""What quadric-error placement of the clustered vertices costs and gains:
rn_mesh_place_quadric with cells of 2 and 4 voxel sides on two meshes, next to rn_mesh_simplify on
the same mesh and grid (whose `cluster` and mean positions it consumes), the two taking turns.

  mrf_128       the MRF's surface of the synthetic scene after a pass at bench.py's shape (128^3)
  fused_256     the mesh fused from that pass's depth maps at 256 x 256 x 128 (fusion_bench's)

One process on one GPU.  Per call of the entry a hipEvent pair on the stream (rn_timer_*), after
`--warmup` calls, min and median over `--repeats`.  Bytes a kernel must move, with nv' the output
vertices (gathers counted once per use; the atomics are counted, not weighed):

  k_quadric_clear     88 nv' written
  k_quadric_members   4 nv read, one 64-bit atomic per clustered vertex
  k_quadric_faces     12 nf read, 36 nf gathered (the corners), 12 nf gathered (cluster), 12 per
                      face and distinct cluster gathered (the mean), up to ten 64-bit atomics per
                      face and distinct cluster (a term that rounds to 0 adds nothing)
  k_quadric_solve     88 nv' read, 12 nv' read, 12 nv' written, two tallies

Recorded, not asserted: the distance of the simplified vertices to the UNSIMPLIFIED surface (the
nearest-surface query of raynet_amd.mesh.MeshRaycaster) under both placements, in cell sides --
RMS, mean, the 99th percentile and the maximum -- and the entry's two counts.  Prints one JSON line
and writes it to profiles/quadric_bench.json.

The kernels cannot be bracketed from outside the entry, so they come out of a kernel trace of
their own:

    python tools/quadric_bench.py [--repeats 30] [--warmup 5]
    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/quadric_bench.py --trace
    python tools/quadric_bench.py --merge_trace DIR/.../*_kernel_trace.csv
    python tools/quadric_bench.py --merge_box FILE      # bench.py's JSON line of the same visit

--trace runs nothing but the warm-ups and repeats of the entry; --merge_trace and --merge_box (no
GPU) add the kernels' own times and the box's speed to the JSON.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_bench as mb  # noqa: E402  (puts the repository on the path)

import numpy as np  # noqa: E402

MESHES = mb.MESHES
CELLS = (2.0, 4.0)
REGULARIZATION, MAX_MOVE = 2.0 ** -10, 1.0
OWN = ("k_quadric_clear", "k_quadric_members", "k_quadric_faces", "k_quadric_solve")


def kernel_bytes(nv, nf, nvo):
    return {"k_quadric_clear": 88 * nvo,
            "k_quadric_members": 4 * nv,
            "k_quadric_faces": 12 * nf + 36 * nf + 12 * nf,
            "k_quadric_solve": 88 * nvo + 24 * nvo}


def distances(surface, positions, cell):
    """The distance of every position to the surface, in sides of the largest cell."""
    dist, _, _ = surface.closest_points(positions)
    d = dist.cpu().numpy() / float(np.max(cell))
    d = d[np.isfinite(d)]
    return {"rms": float(np.sqrt((d ** 2).mean())), "mean": float(d.mean()),
            "p99": float(np.percentile(d, 99)), "max": float(d.max())}


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.hip_implementations.context import _ptr, _stream
    from raynet_amd.mesh import MeshRaycaster
    from raynet_amd.simplify import cluster_grid
    _lib.build()
    found = mb.bench_meshes()
    ctx = get_context()
    res = {"tool": "quadric_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "cells_in_voxel_sides": list(CELLS),
           "regularization": REGULARIZATION, "max_move": MAX_MOVE, "meshes": {}}
    for name in MESHES:
        vertices, faces, voxel = found[name]
        nv, nf = len(vertices), len(faces)
        host = vertices.cpu().numpy()
        vo = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        fo = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
        so, cl = (torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(2))
        counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
        tally = torch.zeros((2,), dtype=torch.int64, device="cuda")
        entry = {"nv": nv, "nf": nf, "voxel": [float(x) for x in voxel], "cells": {}}
        surface = None if args.trace else MeshRaycaster(
            vertices[faces.long().reshape(-1)].reshape(-1, 9))
        for cell in CELLS:
            origin, cell3, dims = cluster_grid(host, cell * voxel)
            o = (ctypes.c_double * 3)(*origin)
            c = (ctypes.c_double * 3)(*cell3)
            d = (ctypes.c_int32 * 3)(*[int(x) for x in dims])
            work = torch.empty((ctx.mesh_simplify_workspace_bytes(nv, nf, dims),),
                               dtype=torch.uint8, device="cuda")

            def simplify():
                ctx._check(ctx.lib.rn_mesh_simplify(
                    ctx._h, nv, _ptr(vertices), nf, _ptr(faces), o, c, d, _ptr(vo), _ptr(fo),
                    _ptr(so), _ptr(cl), _ptr(counts), _ptr(work), _stream()))

            simplify()
            nvo, nfo = (int(x) for x in counts.tolist())
            mean = vo[:nvo].clone()
            placed = torch.empty((nvo, 3), dtype=torch.float32, device="cuda")
            sums = torch.empty((max(ctx.mesh_place_quadric_workspace_bytes(nv, nf, nvo), 8),),
                               dtype=torch.uint8, device="cuda")

            def place():
                ctx._check(ctx.lib.rn_mesh_place_quadric(
                    ctx._h, nv, _ptr(vertices), nf, _ptr(faces), _ptr(cl), nvo, _ptr(mean), c,
                    REGULARIZATION, MAX_MOVE, _ptr(placed), _ptr(tally), _ptr(sums), _stream()))

            launches = {"place_quadric": place, "simplify": simplify}
            if args.trace:
                del launches["simplify"]
            ms = mb.take_turns(ctx, launches, args.warmup, args.repeats)
            if args.trace:
                continue
            per_kernel = kernel_bytes(nv, nf, nvo)
            one = {"dims": [int(x) for x in dims], "nv_out": nvo, "nf_out": nfo,
                   "workspace_bytes": 88 * nvo, "bytes_must_move": per_kernel,
                   "moved": int(tally[0].item()), "fell_back": int(tally[1].item())}
            for k in launches:
                one[k] = mb.stats(ms[k])
            one["place_quadric"]["ratio_to_simplify"] = round(
                one["place_quadric"]["ms_median"] / one["simplify"]["ms_median"], 3)
            one["distance_to_unsimplified_surface_in_cell_sides"] = {
                "mean_placement": distances(surface, mean, cell3),
                "quadric_placement": distances(surface, placed, cell3)}
            move = (placed.double() - mean.double()).abs().cpu().numpy() / cell3
            one["farthest_move_in_cell_sides"] = float(move[np.isfinite(move)].max())
            entry["cells"]["%g" % cell] = one
        res["meshes"][name] = entry
    if args.trace:
        return
    mb.write_record(res, args.out)


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON."""
    res = json.loads(open(args.out).read())
    turns = res["warmup"] + res["repeats"]
    rows = mb.trace_rows(args.merge_trace, OWN)
    settings = [(name, "%g" % cell) for name in MESHES for cell in res["cells_in_voxel_sides"]]
    mb.keep_last(rows, {k: len(settings) * turns for k in OWN})
    for s, (name, cell) in enumerate(settings):
        one = res["meshes"][name]["cells"][cell]
        own = {}
        for k in OWN:
            mine = rows[k][s * turns:(s + 1) * turns][res["warmup"]:]
            own[k] = mb.stats([(e - b) * 1e-6 for b, e in mine])
            own[k]["GB_per_s"] = round(one["bytes_must_move"][k] / (own[k]["ms_median"] * 1e-3) / 1e9, 1)
        own["sum_of_kernels_ms"] = round(sum(own[k]["ms_median"] for k in OWN), 4)
        one["kernel_trace"] = own
    mb.write_record(res, args.out)


if __name__ == "__main__":
    mb.main("quadric_bench", measure, merge_trace)
