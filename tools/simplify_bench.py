#!/usr/bin/env python3
"""What vertex clustering of a mesh costs: rn_mesh_simplify with cells of 2
and 4 voxel sides on two meshes, against rn_mesh_components on the same mesh (this chain's other
multi-launch, atomics-bound entry), the two taking turns.

  mrf_128       the MRF's surface of the synthetic scene after a pass at bench.py's shape (128^3)
  fused_256     the mesh fused from that pass's depth maps at 256 x 256 x 128 (fusion_bench's)

One process on one GPU.  Per call of the entry a hipEvent pair on the stream (rn_timer_*), after
`--warmup` calls, min and median over `--repeats`.  Bytes a kernel must move, with C cells, nv' and
nf' the outputs (gathers counted once per use; the atomics are counted, not weighed):

  k_simplify_clear          32 C written
  k_simplify_bin            12 nv read, 12 nv written (cell_of, the flag), 5 atomics per binned vertex
  k_simplify_face_flags     12 nf read, 24 nf gathered (cell_of, rep), 8 nf + 24 nf' written
  the two scans             24 (nf + nv): a reduce pass and a read-write pass per level-0 word
  k_simplify_emit_vertices  4 nv read, 20 nv gathered (rep, two scan words), 4 nv written, and per
                            output vertex 16 of the table, 12 read, 16 written
  k_simplify_emit_faces     12 nf read, 24 nf gathered, 8 nf read (the scan), 24 nf' gathered, 12 nf'
                            written

Also: the share of duplicate faces `unique_faces` finds in the output, and what ten smoothing
iterations (rn_mesh_smooth) cost on the simplified mesh against the unsimplified one -- the
downstream saving.  Prints one JSON line and writes it to profiles/simplify_bench.json.

The kernels cannot be bracketed from outside the entry, so they come out of a kernel trace of
their own:

    python tools/simplify_bench.py [--repeats 30] [--warmup 5]
    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/simplify_bench.py --trace
    python tools/simplify_bench.py --merge_trace DIR/.../*_kernel_trace.csv
    python tools/simplify_bench.py --merge_box FILE      # bench.py's JSON line of the same visit

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
SMOOTH_ITERATIONS = 10
OWN = ("k_simplify_clear", "k_simplify_bin", "k_simplify_face_flags", "k_simplify_emit_vertices",
       "k_simplify_emit_faces")


def scan_launches(n):
    """(reduce launches, tile launches) of the grid-level scan of n words."""
    levels = 1
    while n > 256:
        n = (n + 255) // 256
        levels += 1
    return levels - 1, levels


def kernel_bytes(nv, nf, cells, nvo, nfo):
    return {"k_simplify_clear": 32 * cells,
            "k_simplify_bin": 24 * nv,
            "k_simplify_face_flags": 12 * nf + 24 * nf + 8 * nf + 24 * nfo,
            "scans": 24 * (nf + nv),
            "k_simplify_emit_vertices": 4 * nv + 20 * nv + 4 * nv + 44 * nvo,
            "k_simplify_emit_faces": 12 * nf + 24 * nf + 8 * nf + 36 * nfo}


def time_smoothing(ctx, vertices, faces, args):
    import torch
    from raynet_amd.appearance import corner_table
    from raynet_amd.smoothing import boundary_vertices
    nv, nf = len(vertices), len(faces)
    offsets, corners = corner_table(faces, nv)
    fixed = boundary_vertices(faces, nv).to(torch.uint8)
    work = torch.empty((max(ctx.mesh_smooth_workspace_bytes(nv, nf), 8),), dtype=torch.uint8,
                       device="cuda")
    out = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    ms = mb.take_turns(ctx, {"smooth": lambda: ctx.mesh_smooth(
        vertices, faces, offsets, corners, fixed, SMOOTH_ITERATIONS, 0.5, -0.53, float("inf"), work,
        out)}, args.warmup, args.repeats)
    return mb.stats(ms["smooth"])


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.hip_implementations.context import _ptr, _stream
    from raynet_amd.simplify import cluster_grid, unique_faces
    _lib.build()
    found = mb.bench_meshes()
    ctx = get_context()
    res = {"tool": "simplify_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "cells_in_voxel_sides": list(CELLS),
           "smooth_iterations": SMOOTH_ITERATIONS, "meshes": {}}
    for name in MESHES:
        vertices, faces, voxel = found[name]
        nv, nf = len(vertices), len(faces)
        host = vertices.cpu().numpy()
        labels, vc, fc = (torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(3))
        status = torch.zeros((1,), dtype=torch.int32, device="cuda")
        vo = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        fo = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
        so, cl = (torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(2))
        counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
        entry = {"nv": nv, "nf": nf, "voxel": [float(x) for x in voxel], "cells": {}}
        if not args.trace:
            entry["smooth_unsimplified"] = time_smoothing(ctx, vertices, faces, args)
        for cell in CELLS:
            origin, cell3, dims = cluster_grid(host, cell * voxel)
            o = (ctypes.c_double * 3)(*origin)
            c = (ctypes.c_double * 3)(*cell3)
            d = (ctypes.c_int32 * 3)(*[int(x) for x in dims])
            work = torch.empty((ctx.mesh_simplify_workspace_bytes(nv, nf, dims),),
                               dtype=torch.uint8, device="cuda")
            launches = {
                "simplify": lambda: ctx._check(ctx.lib.rn_mesh_simplify(
                    ctx._h, nv, _ptr(vertices), nf, _ptr(faces), o, c, d, _ptr(vo), _ptr(fo),
                    _ptr(so), _ptr(cl), _ptr(counts), _ptr(work), _stream())),
                "components": lambda: ctx._check(ctx.lib.rn_mesh_components(
                    ctx._h, nv, nf, _ptr(faces), _ptr(labels), _ptr(vc), _ptr(fc), _ptr(status),
                    _stream())),
            }
            if args.trace:
                del launches["components"]
            ms = mb.take_turns(ctx, launches, args.warmup, args.repeats)
            if args.trace:
                continue
            nvo, nfo = (int(x) for x in counts.tolist())
            cells = int(np.prod(dims.astype(np.int64)))
            per_kernel = kernel_bytes(nv, nf, cells, nvo, nfo)
            total = sum(per_kernel.values())
            one = {"dims": [int(x) for x in dims], "table_cells": cells,
                   "workspace_bytes": int(work.numel()), "nv_out": nvo, "nf_out": nfo,
                   "face_reduction": round(nf / max(nfo, 1), 2),
                   "vertex_reduction": round(nv / max(nvo, 1), 2),
                   "bytes_must_move": per_kernel}
            for k in launches:
                one[k] = mb.stats(ms[k])
            one["simplify"]["GB_per_s"] = round(total / (one["simplify"]["ms_median"] * 1e-3) / 1e9, 1)
            one["simplify"]["ratio_to_components"] = round(
                one["simplify"]["ms_median"] / one["components"]["ms_median"], 3)
            single = unique_faces(fo[:nfo])
            one["duplicate_face_share"] = round(1.0 - len(single) / max(nfo, 1), 5)
            one["nf_out_unique"] = len(single)
            if len(single):
                one["smooth_simplified"] = time_smoothing(
                    ctx, vo[:nvo].contiguous(), single.contiguous(), args)
                one["smooth_saving"] = round(entry["smooth_unsimplified"]["ms_median"] /
                                             one["smooth_simplified"]["ms_median"], 2)
            entry["cells"]["%g" % cell] = one
        res["meshes"][name] = entry
    if args.trace:
        return
    mb.write_record(res, args.out)


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON."""
    res = json.loads(open(args.out).read())
    turns = res["warmup"] + res["repeats"]
    names = OWN + ("k_scan_reduce", "k_scan_tile")
    rows = mb.trace_rows(args.merge_trace, names)
    at = {k: 0 for k in names}
    # the turns are the last dispatches of the run (the scan also serves the meshes' extraction,
    # which came before): walk backwards from the end of every kernel's list
    plan = []
    for name in MESHES:
        entry = res["meshes"][name]
        reduce_n, tile_n = (sum(x) for x in zip(scan_launches(entry["nf"]), scan_launches(entry["nv"])))
        for cell in res["cells_in_voxel_sides"]:
            per_turn = {k: 1 for k in OWN}
            per_turn.update(k_scan_reduce=reduce_n, k_scan_tile=tile_n)
            plan.append((name, "%g" % cell, per_turn))
    mb.keep_last(rows, {k: sum(p[2][k] for p in plan) * turns for k in names})
    for name, cell, per_turn in plan:
        own = {}
        one = res["meshes"][name]["cells"][cell]
        for k in names:
            p = per_turn[k]
            mine = rows[k][at[k]:at[k] + p * turns]
            at[k] += p * turns
            sums = [sum((e - s) * 1e-6 for s, e in mine[i * p:(i + 1) * p]) for i in range(turns)]
            own[k] = mb.stats(sums[res["warmup"]:])
            own[k]["launches"] = p
        scans = own["k_scan_reduce"]["ms_median"] + own["k_scan_tile"]["ms_median"]
        own["scans"] = {"ms_median": round(scans, 4)}
        for k in OWN + ("scans",):
            own[k]["GB_per_s"] = round(one["bytes_must_move"][k] / (own[k]["ms_median"] * 1e-3) / 1e9, 1)
        own["sum_of_kernels_ms"] = round(sum(own[k]["ms_median"] for k in OWN) + scans, 4)
        one["kernel_trace"] = own
    mb.write_record(res, args.out)


if __name__ == "__main__":
    mb.main("simplify_bench", measure, merge_trace)
