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
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_bench as mb  # noqa: E402  (puts the repository on the path)

import numpy as np  # noqa: E402

STRIP = 2000000
MESHES = mb.MESHES + ("strip_2m",)
KERNELS = ("k_cc_init", "k_cc_hook", "k_cc_flatten", "k_cc_count")


def meshes():
    """-> {name: (vertices (nv, 3) f32 device, faces (nf, 3) i32 device)}: the two every mesh
    bench measures on, and the strip."""
    import torch
    out = {k: (v, f) for k, (v, f, _) in mb.bench_meshes().items()}
    rng = np.random.default_rng(7)
    order = rng.permutation(STRIP).astype(np.int32)
    i = np.arange(STRIP - 2)
    faces = np.stack([order[i], order[i + 1], order[i + 2]], 1)[rng.permutation(STRIP - 2)]
    out["strip_2m"] = (torch.from_numpy(rng.normal(size=(STRIP, 3)).astype(np.float32)).cuda(),
                       torch.from_numpy(np.ascontiguousarray(faces, dtype=np.int32)).cuda())
    return out


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
        sys.path.insert(0, os.path.join(mb.REPO, "tests"))
        import components_truth as ct
        t0 = time.perf_counter()
        labels = ct.labels_of(faces, nv)
        return "tests/components_truth.py", time.perf_counter() - t0, len(np.unique(labels))


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
        ms = mb.take_turns(ctx, launches, args.warmup, args.repeats)
        if int(status.item()) != 0:
            raise SystemExit("%s: the status word is %d" % (name, int(status.item())))
        if args.trace:
            continue
        labels = outs[0].cpu().numpy()
        K = int((labels == np.arange(nv)).sum())
        must_move = 12 * nf + 12 * nv
        out = {"nv": nv, "nf": nf, "K": K, "bytes_must_move": must_move}
        for k in launches:
            out[k] = mb.stats(ms[k])
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
    mb.write_record(res, args.out)


def merge_trace(args):
    """The kernels' own times out of a rocprofv3 kernel trace of `--trace`, into the JSON."""
    res = json.loads(open(args.out).read())
    per_mesh = res["warmup"] + res["repeats"]
    rows = mb.keep_last(mb.trace_rows(args.merge_trace, KERNELS),
                        {k: per_mesh * len(MESHES) for k in KERNELS}, exact=True)
    for at, name in enumerate(MESHES):
        own = {}
        for k in KERNELS:
            mine = rows[k][at * per_mesh + res["warmup"]:(at + 1) * per_mesh]
            own[k] = mb.stats([(e - s) * 1e-6 for s, e in mine])
        first = rows["k_cc_init"][at * per_mesh + res["warmup"]:(at + 1) * per_mesh]
        last = rows["k_cc_count"][at * per_mesh + res["warmup"]:(at + 1) * per_mesh]
        own["first_start_to_last_end"] = mb.stats([(e[1] - s[0]) * 1e-6 for s, e in zip(first, last)])
        res["meshes"][name]["kernel_trace"] = own
    mb.write_record(res, args.out)


if __name__ == "__main__":
    mb.main("components_bench", measure, merge_trace)
