#!/usr/bin/env python3
"""Steady-state assembly of a mixed-view training batch, two ways in one process, and its share
of a training step.

    python tools/batch_bench.py [--rays 1000] [--views 40] [--repeat 20] [--out profiles/train_batch_bench.json]

A synthetic scene at the reference's training defaults (1000 rays, D = 32, N = 5, 11 x 11 x 3
patches, 40 views on an arc looking at a textured ground plane inside the box):

  new      train_network/ray_sampler.py: rn_batch_rays on all candidates, compaction, traversal
           and targets of the kept rays, rn_batch_patches;
  grouped  what the code before it offers for the SAME candidates: group them by reference view,
           target_points_for_rays + get_batch_of_rays per group (unchanged code);
  step     sampler.next_batch() + Trainer.train_step, with assembly's share of it.

Wall-clock times around a device synchronisation, medians over --repeat runs after 3 warm-up
runs, the two assembly routes alternating; only the comparison within one process means anything.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

GROUND_Z = -0.4


def make_scene(views, H, W):
    from raynet_amd.common.scene import Image, Scene
    from raynet_amd.synthetic import ring_cameras
    cams = ring_cameras(views, H, W, radius=3.0, focal=1.6 * H, arc=0.5 * np.pi,
                        heights=[1.6 + 0.01 * v for v in range(views)])
    images, depth = [], []
    py, px = np.mgrid[0:H, 0:W]
    pix = np.stack([px.ravel(), py.ravel(), np.ones(H * W)]).astype(np.float64)
    for cam in cams:
        o = np.asarray(cam.P_pinv, np.float64).dot(pix)
        c = np.asarray(cam.center, np.float64).ravel()[:3]
        d = o[:3] / o[3] - c[:, None]
        d /= np.linalg.norm(d, axis=0)
        t = (GROUND_Z - c[2]) / d[2]
        X = c[:, None] + t * d
        tex = np.stack([0.5 + 0.5 * np.sin(7 * X[0] + 3 * X[1]), 0.5 + 0.5 * np.sin(9 * X[1] - 4 * X[0]),
                        0.5 + 0.5 * np.cos(11 * X[0] * X[1])], -1).astype(np.float32)
        images.append(Image(tex.reshape(H, W, 3), cam))
        depth.append(np.where(t > 0, t, 0).astype(np.float32).reshape(H, W))
    scene = Scene(images, (-1, -1, -1, 1, 1, 1))
    scene.get_depth_map = lambda i: depth[i]
    return scene


class OneScene(object):
    n_scenes = 1

    def __init__(self, scene):
        self._scene = scene

    def get_scene(self, i):
        return self._scene


def median_ms(fn, repeat, warmup=3):
    import torch
    times = []
    for i in range(warmup + repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def alternating_ms(a, b, repeat, warmup=2):
    """The two routes in turn, so that whatever else the machine does hits both alike."""
    import torch
    ta, tb = [], []
    for i in range(warmup + repeat):
        for fn, times in ((a, ta), (b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times.append((time.perf_counter() - t0) * 1e3)
    return tuple((float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in (ta, tb))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--rays", type=int, default=1000)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--image", default="240,320")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.models import get_nn
    from raynet_amd.train_network import ray_sampler as rs
    from raynet_amd.train_network.raynet_batch_provider import (get_batch_of_rays,
                                                                 target_points_for_rays)
    from raynet_amd.train_network.trainer import Trainer
    H, W = (int(v) for v in args.image.split(","))
    D, N, M, grid, patch = 32, 5, 160, (64, 64, 32), (11, 11)
    scene = make_scene(args.views, H, W)
    gp = GenerationParameters(depth_planes=D, neighbors=N - 1, grid_shape=np.array(grid, np.int32),
                              max_number_of_marched_voxels=M, padding=11)
    bank = rs.SceneBank(OneScene(scene), gp)
    sampler = rs.RayBatchSampler(bank, args.rays, mode="random", window=4, seed=0)
    entry = bank.get(0)
    first = sampler.next_batch()                       # settles the acceptance estimate
    acceptance = sampler._acceptance

    # ---- the same candidates for both routes: as many as the sampler would draw
    rng = np.random.default_rng(1)
    m = int(np.ceil(args.rays / acceptance * 1.25)) + 32
    view = rng.integers(2, args.views - 4, m).astype(np.int32)
    ridx = rng.integers(0, H * W, m).astype(np.int32)

    def new_route():
        return rs.assemble(entry, entry.hip.dev(view), entry.hip.dev(ridx), patch, reject=True)

    images = {v: entry.images[v].permute(2, 0, 1).contiguous() for v in range(args.views)}

    def grouped_route():
        out = []
        for v in np.unique(view):
            r = ridx[view == v]
            points, valid = target_points_for_rays(scene, int(v), r)
            if valid.any():
                out.append(get_batch_of_rays(scene, int(v), r[valid], gp, entry.hip, images,
                                             points[valid], patch))
        return out

    kept_new = len(new_route())
    kept_grouped = sum(len(b[N + 1]) for b in grouped_route())
    t_new, t_grouped = alternating_ms(new_route, grouped_route, args.repeat)
    t_sampler = median_ms(sampler.next_batch, args.repeat)

    # ---- a training step on such batches
    model = get_nn("simple_cnn")().cuda()
    trainer = Trainer(model, "raynet", N, "/nonexistent", loss="squared_emd", lr=1e-3, clipnorm=0.1,
                      train_with_gamma=True)
    batch = sampler.next_batch()
    t_step = median_ms(lambda: trainer.train_step(batch), args.repeat)
    t_both = median_ms(lambda: trainer.train_step(sampler.next_batch()), args.repeat)

    result = {
        "device": torch.cuda.get_device_name(0), "rays": args.rays, "views": args.views,
        "image": [H, W], "D": D, "N": N, "patch": list(patch) + [3], "candidates": m,
        "distinct_reference_views": int(len(np.unique(view))), "acceptance": acceptance,
        "kept_new": kept_new, "kept_grouped": kept_grouped, "first_batch_rays": len(first),
        "assemble_new_ms": t_new[0], "assemble_new_min_max_ms": t_new[1:],
        "assemble_grouped_ms": t_grouped[0], "assemble_grouped_min_max_ms": t_grouped[1:],
        "grouped_over_new": t_grouped[0] / t_new[0],
        "sampler_next_batch_ms": t_sampler[0], "train_step_ms": t_step[0],
        "next_batch_plus_step_ms": t_both[0],
        "assembly_share_of_loop": t_sampler[0] / t_both[0],
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
