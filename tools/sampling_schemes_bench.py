#!/usr/bin/env python3
"""What the sampling schemes cost in the plane sweep: K10 -- sample,
sweep, arg-max plane, depth -- per image at 1280 x 720, 5 views, D = 32, F = 32, for
sample_in_bbox, sample_in_range and sample_in_disparity in one process on one GPU.  Prints one
JSON line and writes it to profiles/sampling_schemes_bench.json.

sample_in_bbox runs through the OLD entry (rn_mvcnn_depth: two rays per wavefront at D = 32), the
other two through rn_mvcnn_depth_scheme (one ray per wavefront; sample_in_disparity with lane k's
fp64 construction of its point).  The synthetic scene is bench.py's ring of cameras around the box
[-1, 1]^3 with planted feature maps; the range is (2, 4).  All H * W rays of an image are one
launch; a figure is the median over `--repeats` launches (hipEvents around each, after
`--warmup`), the schemes taking turns, for every one of the 5 reference images, and the median of
those five.

    python tools/sampling_schemes_bench.py [--repeats 10] [--warmup 3]
    python tools/sampling_schemes_bench.py --tree OTHER_CHECKOUT --out ''    # its bbox figure only

--tree: another (built) checkout of this repository, e.g. the parent commit: only sample_in_bbox
is timed, with that checkout's package and library.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, V, D, F, PAD = 720, 1280, 5, 32, 32, 11
RANGE = (2.0, 4.0)
SCHEMES = ("sample_in_bbox", "sample_in_range", "sample_in_disparity")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sampling_schemes_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else REPO)
    import numpy as np
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.synthetic import make_synthetic_scene
    if not args.tree:
        _lib.build()
    schemes = SCHEMES[:1] if args.tree else SCHEMES
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=V, F=F, padding=PAD, focal=1.5 * H)
    ctx = get_context(1, D, V, F, H, W, PAD, np.asarray(scene.bbox, np.float32).ravel(), (1, 1, 1))
    n = H * W
    ridx = torch.arange(n, dtype=torch.int32, device="cuda")
    S = torch.empty((n, D), device="cuda")
    pts = torch.empty((n, D, 4), device="cuda")
    depth = torch.empty((n,), device="cuda")
    per_image = {s: [] for s in schemes}
    missed = []
    for ref in range(V):
        views = scene.view_indices_with_neighbors(ref, V - 1)
        cams = [scene.get_image(v).camera for v in views]
        feats = bank.stacked(views)
        P = ctx.dev(np.ascontiguousarray(np.array([c.P for c in cams], np.float32)))
        P_inv = ctx.dev(np.ascontiguousarray(cams[0].P_pinv, dtype=np.float32))
        centre = ctx.dev(np.asarray(cams[0].center, np.float32).ravel())

        def run(scheme):
            if scheme == "sample_in_bbox":
                ctx.mvcnn_depth(ridx, feats, P, P_inv, centre, S, pts, depth)
            else:
                sm = ctx.sampling(scheme, RANGE, (cams[-1].P, cams[-1].P_pinv, cams[-1].center))
                ctx.mvcnn_depth_scheme(ridx, feats, P, P_inv, centre, sm, S, pts, depth)
        for _ in range(args.warmup):
            for s in schemes:
                run(s)
        ms = {s: [] for s in schemes}
        for _ in range(args.repeats):
            for s in schemes:
                ctx.timer_start()
                run(s)
                ms[s].append(ctx.timer_stop())
        for s in schemes:
            per_image[s].append(float(np.median(ms[s])))
        if "sample_in_disparity" in schemes:
            missed.append(int((pts[:, 0, 3] == 0).sum()))        # (the last scheme run)
    out = {"tool": "sampling_schemes_bench", "device": torch.cuda.get_device_name(0),
           "version": _lib.load().rn_version().decode(), "tree": args.tree,
           "shape": dict(H=H, W=W, views=V, D=D, F=F, padding=PAD, range=RANGE),
           "repeats": args.repeats, "warmup": args.warmup,
           "k10_ms_per_image": {s: round(float(np.median(per_image[s])), 4) for s in schemes},
           "k10_ms_by_reference_image": {s: [round(x, 4) for x in per_image[s]] for s in schemes},
           "disparity_rays_missing_the_box": missed}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
