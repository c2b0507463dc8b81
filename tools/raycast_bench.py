#!/usr/bin/env python3
"""Timing of the ground-truth mesh ray cast (raynet_amd/mesh.py) on one GPU: prints one JSON
line.  For synthetic box cities (raynet_amd.synthetic.make_box_city) of 1e5, 1e6 and 4e6
triangles: the BVH build (ms, synchronised wall time: Morton keys, sort, hierarchy, boxes,
depth check) and full 1280 x 720 depth maps of the 12 mock cameras
(tests/golden/restrepo_mock_scene_1), timed with hipEvents after one warm-up pass:
ms per map and rays per second.

    python tools/raycast_bench.py [--sizes 100000,1000000,4000000] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,4000000")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from raynet_amd import _lib
    from raynet_amd.common.camera import Camera
    from raynet_amd.common.scene import read_krt
    from raynet_amd.mesh import MeshRaycaster
    from raynet_amd.synthetic import make_box_city
    _lib.build()
    mock = os.path.join(REPO, "tests", "golden", "restrepo_mock_scene_1", "cams_krt")
    cams = [Camera(*read_krt(os.path.join(mock, c))) for c in sorted(os.listdir(mock))]
    H, W = 720, 1280
    out = {"tool": "raycast_bench", "device": torch.cuda.get_device_name(0),
           "image": [H, W], "cameras": len(cams), "meshes": []}
    for n in [int(s) for s in args.sizes.split(",")]:
        tri = make_box_city(n, seed=1)
        tri_dev = torch.from_numpy(tri).cuda()
        MeshRaycaster(tri_dev)                      # warm-up (module load, allocator)
        torch.cuda.synchronize()
        builds = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            rc = MeshRaycaster(tri_dev)
            torch.cuda.synchronize()
            builds.append((time.perf_counter() - t0) * 1e3)
        for cam in cams:                            # warm-up pass
            rc.depth_map(cam, H, W)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per_pass = []
        for _ in range(args.repeats):
            start.record()
            for cam in cams:
                D = rc.depth_map(cam, H, W)
            stop.record()
            stop.synchronize()
            per_pass.append(start.elapsed_time(stop))
        ms_map = float(np.median(per_pass)) / len(cams)
        hit = float((D > 0).float().mean().item())
        out["meshes"].append({
            "triangles": int(len(tri)), "bvh_depth": rc.depth,
            "build_ms": round(float(np.median(builds)), 3),
            "ms_per_map": round(ms_map, 3),
            "rays_per_s": round(H * W / (ms_map * 1e-3), 1),
            "hit_fraction_last_map": round(hit, 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
