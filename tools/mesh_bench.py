"""What the bench tools of the mesh stages share ({components,smooth,simplify,holes}_bench.py): the
two meshes every one of them measures on, the turn-about timing loop, the reading of a rocprofv3
kernel trace, the JSON record and the command line.  Nothing here needs torch or a GPU until
bench_meshes() or take_turns() is called, so the merge halves of the tools run without either."""
import argparse
import csv
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

H, W, V, NEIGHBORS, D, M = 480, 640, 5, 4, 64, 384
GRID, FUSED_GRID, THRESHOLD = (128, 128, 128), (256, 256, 128), 0.5
MESHES = ("mrf_128", "fused_256")


def bench_meshes():
    """One synthetic pass at bench.py's shape -> {name: (vertices (nv, 3) f32 device, faces (nf, 3)
    i32 device, the voxel's sides [3])} for mrf_128, the MRF's surface at 128^3, and fused_256, the
    mesh fused from that pass's depth maps at 256 x 256 x 128."""
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
    mrf = fp.occupancy_volume()
    fused = fuse_scene(scene, [m for m, _ in pairs], range(V), FUSED_GRID,
                       weights=[c for _, c in pairs])
    out = {}
    for name, volume, mesh in (("mrf_128", mrf, mrf.mesh(THRESHOLD)),
                               ("fused_256", fused, fused.mesh())):
        bbox = np.asarray(volume.bbox, np.float64)
        voxel = (bbox[3:] - bbox[:3]) / np.array(volume.grid_shape, np.float64)
        out[name] = (torch.from_numpy(np.ascontiguousarray(mesh.vertices)).cuda(),
                     torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int32)).cuda(), voxel)
    return out


def stats(ms):
    return {"ms_min": round(float(min(ms)), 4), "ms_median": round(float(np.median(ms)), 4)}


def take_turns(ctx, launches, warmup, repeats):
    """The launches {name: callable} taking turns, warmup + repeats times, each call between a
    hipEvent pair on the stream -> {name: the milliseconds of the repeats}."""
    import torch
    ms = {k: [] for k in launches}
    for _ in range(warmup + repeats):
        for k, f in launches.items():
            ctx.timer_start()
            f()
            ms[k].append(ctx.timer_stop())
    torch.cuda.synchronize()
    return {k: v[warmup:] for k, v in ms.items()}


def trace_rows(csv_path, kernel_names):
    """A rocprofv3 kernel_trace.csv -> {kernel: [(start, end)] in ns, ascending} for the kernels
    whose names contain one of kernel_names."""
    rows = {k: [] for k in kernel_names}
    with open(csv_path) as f:
        for row in csv.DictReader(f):
            for k in kernel_names:
                if k in row["Kernel_Name"]:
                    rows[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for k in kernel_names:
        rows[k].sort()
    return rows


def keep_last(rows, expected, exact=False):
    """The turns are the last dispatches of the run (whatever built the meshes came before): of
    every kernel's rows the last expected[kernel], in place.  Fewer than that -- with exact, any
    other number -- ends the program."""
    for k, n in expected.items():
        if len(rows[k]) != n if exact else len(rows[k]) < n:
            raise SystemExit("%s: %d dispatches in the trace, expected %d" % (k, len(rows[k]), n))
        rows[k] = rows[k][len(rows[k]) - n:]
    return rows


def write_record(res, out):
    """The record as one JSON line: printed, and written to `out` if that is given."""
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def merge_box(args):
    """bench.py's JSON line of the same visit, under "box"."""
    res = json.loads(open(args.out).read())
    lines = [l for l in open(args.merge_box).read().splitlines() if l.strip().startswith("{")]
    res["box"] = json.loads(lines[-1])
    write_record(res, args.out)


def main(tool, measure, merge_trace):
    """The command line the four tools share: measure(args) on the GPU, or one of the merges."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true",
                    help="only the entry's launches (for a kernel trace); writes nothing")
    ap.add_argument("--merge_trace", default=None,
                    help="a rocprofv3 kernel_trace.csv of --trace: add the kernels' times (no GPU)")
    ap.add_argument("--merge_box", default=None,
                    help="a file with bench.py's JSON line of the same visit (no GPU)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", tool + ".json"))
    args = ap.parse_args()
    if args.merge_trace:
        merge_trace(args)
    elif args.merge_box:
        merge_box(args)
    else:
        measure(args)
