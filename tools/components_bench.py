#!/usr/bin/env python3
"""What labelling the connected components of a mesh costs:
rn_mesh_components on three meshes against rn_vertex_area_normals on the same mesh (one pass over
the same faces; with the corner table it needs, and alone) and against a union-find on the host.

  mrf_128       the MRF's surface of the synthetic scene after a pass at bench.py's shape (128^3)
  fused_256     the mesh fused from that pass's depth maps at 256 x 256 x 128 (fusion_bench's)
  strip_2m      the strip (i, i + 1, i + 2) over 2 M vertices, ids permuted and faces shuffled: the
                deepest chase there is, with no locality at all -- the adversarial case

One process on one GPU.  Per launch of the entry a hipEvent pair on the stream (rn_timer_*), after
`--warmup` launches, min and median over `--repeats`; "must move" is 12 nf + 12 nv bytes, the
faces read once and the three outputs written once.  Prints one JSON line and writes it to
profiles/components_bench.json.

k_cc_hook alone cannot be bracketed from outside the entry, so it comes out of a kernel trace of
its own:

    python tools/components_bench.py [--repeats 30] [--warmup 5]
    rocprofv3 --kernel-trace -f csv -d DIR -- python tools/components_bench.py --trace
    python tools/components_bench.py --merge_trace DIR/.../*_kernel_trace.csv

--trace runs nothing but the meshes' warm-ups and repeats of the entry; --merge_trace (no GPU)
adds the four kernels' own times per mesh to the JSON.
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
STRIP = 2000000
MESHES = ("mrf_128", "fused_256", "strip_2m")
KERNELS = ("k_cc_init", "k_cc_hook", "k_cc_flatten", "k_cc_count")


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
    rng = np.random.default_rng(7)
    order = rng.permutation(STRIP).astype(np.int32)
    i = np.arange(STRIP - 2)
    faces = np.stack([order[i], order[i + 1], order[i + 2]], 1)[rng.permutation(STRIP - 2)]
    out["strip_2m"] = (rng.normal(size=(STRIP, 3)).astype(np.float32), faces)
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).cuda(),
                torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32)).cuda())
            for k, (v, f) in out.items()}


def host_components(faces, nv):
    """-> (what ran, seconds, the number of components) on the host."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        t0 = time.perf_counter()
        rows = np.concatenate([faces[:, 0], faces[:, 1]])
        cols = np.concatenate([faces[:, 1], faces[:, 2]])
        graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv)).tocsr()
        k, _ = connected_components(graph, directed=False)
        return "scipy.sparse.csgraph.connected_components", time.perf_counter() - t0, int(k)
    except ImportError:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import components_truth as ct
        t0 = time.perf_counter()
        labels = ct.labels_of(faces, nv)
        return "tests/components_truth.py", time.perf_counter() - t0, len(np.unique(labels))


def stats(ms):
    return {"ms_min": round(float(min(ms)), 4), "ms_median": round(float(np.median(ms)), 4)}


def measure(args):
    import torch
    from raynet_amd import _lib
    from raynet_amd.appearance import corner_table
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.hip_implementations.context import _ptr, _stream
    _lib.build()
    found = meshes()
    ctx = get_context()
    res = {"tool": "components_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "repeats": args.repeats,
           "warmup": args.warmup, "meshes": {}}
    for name in MESHES:
        vertices, faces = found[name]
        nv, nf = len(vertices), len(faces)
        outs = [torch.empty((nv,), dtype=torch.int32, device="cuda") for _ in range(3)]
        normals = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
        table = corner_table(faces, nv)
        status = torch.zeros((1,), dtype=torch.int32, device="cuda")

        def components():
            # (the entry itself: the wrapper reads the status word back, a host round trip)
            ctx._check(ctx.lib.rn_mesh_components(ctx._h, nv, nf, _ptr(faces), _ptr(outs[0]),
                                                  _ptr(outs[1]), _ptr(outs[2]), _ptr(status),
                                                  _stream()))

        launches = {
            "components": components,
            "normals_with_corner_table": lambda: ctx.vertex_area_normals(
                vertices, faces, *corner_table(faces, nv), normals),
            "normals_alone": lambda: ctx.vertex_area_normals(vertices, faces, *table, normals),
        }
        if args.trace:
            launches = {"components": launches["components"]}
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
        if int(status.item()) != 0:
            raise SystemExit("%s: the status word is %d" % (name, int(status.item())))
        if args.trace:
            continue
        labels = outs[0].cpu().numpy()
        K = int((labels == np.arange(nv)).sum())
        must_move = 12 * nf + 12 * nv
        out = {"nv": nv, "nf": nf, "K": K, "bytes_must_move": must_move}
        for k in launches:
            out[k] = stats(ms[k])
        out["components"]["GB_per_s"] = round(
            must_move / (out["components"]["ms_median"] * 1e-3) / 1e9, 1)
        for k in ("normals_with_corner_table", "normals_alone"):
            out["components"]["ratio_to_" + k] = round(
                out["components"]["ms_median"] / out[k]["ms_median"], 3)
        what, seconds, host_K = host_components(faces.cpu().numpy(), nv)
        out["host"] = {"what": what, "ms": round(seconds * 1e3, 1), "K": host_K}
        largest = int(outs[2].max().item())
        out["largest_component_faces"] = largest
        res["meshes"][name] = out
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
    per_mesh = res["warmup"] + res["repeats"]
    rows = {k: [] for k in KERNELS}
    with open(args.merge_trace) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for k in KERNELS:
        rows[k].sort()
        if len(rows[k]) != per_mesh * len(MESHES):
            raise SystemExit("%s: %d dispatches in the trace, expected %d"
                             % (k, len(rows[k]), per_mesh * len(MESHES)))
    for at, name in enumerate(MESHES):
        own = {}
        for k in KERNELS:
            mine = rows[k][at * per_mesh + res["warmup"]:(at + 1) * per_mesh]
            own[k] = stats([(e - s) * 1e-6 for s, e in mine])
        first = rows["k_cc_init"][at * per_mesh + res["warmup"]:(at + 1) * per_mesh]
        last = rows["k_cc_count"][at * per_mesh + res["warmup"]:(at + 1) * per_mesh]
        own["first_start_to_last_end"] = stats([(e[1] - s[0]) * 1e-6 for s, e in zip(first, last)])
        res["meshes"][name]["kernel_trace"] = own
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true",
                    help="only launch the entry (for a kernel trace); writes nothing")
    ap.add_argument("--merge_trace", default=None,
                    help="a rocprofv3 kernel_trace.csv of --trace: add the kernels' times (no GPU)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "components_bench.json"))
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
