#!/usr/bin/env python3
"""Golden vectors for the point-cloud filters from the REFERENCE's own code
(raynet/metrics.py:27-127: VoxelMask, ReduceDensity).

Runs only where the reference's sources are present (RAYNET_REFERENCE, default /root/reference)
and scikit-learn is installed.  The sources are converted with lib2to3 into a scratch directory
under /tmp, never into this repository, exactly as gen_pointcloud_from_reference.py does (its
loader is used).  The reference names `np.bool`, which NumPy has removed: the alias is set
before the call.  Its ReduceDensity shuffles np.arange(N) with the global NumPy generator:
`np.random.seed(s)` before each call makes the run repeatable, and the order the same seed
gives np.arange(N) under np.random.shuffle is stored next to the output.

Outputs: tests/golden/ref_filters.npz -- arrays only: points (3, N) float64, bbox (1, 6)
float32, mask (6, 5, 8) uint8, min_dist, shuffle_seed, order (N,), voxel_mask_points,
reduce_density_points, and the same thinning for a second seed (order2, reduce_density_points2).
"""
import os
import shutil

import numpy as np

from gen_pointcloud_from_reference import HERE, load_reference


def main():
    _, metrics, _, scratch = load_reference()
    np.bool = bool
    rng = np.random.default_rng(23)
    n = 3000
    bbox = np.array([[-0.6, -0.5, -0.4, 0.9, 0.75, 0.8]], np.float32)
    mask = (rng.random((6, 5, 8)) < 0.6).astype(np.uint8)
    lo, hi = bbox[0, :3].astype(np.float64), bbox[0, 3:].astype(np.float64)
    # a noisy sphere cap and a slab of uniform points, some of them outside the box
    sphere = rng.standard_normal((3, n // 2))
    sphere = 0.45 * sphere / np.linalg.norm(sphere, axis=0) + 0.01 * rng.standard_normal((3, n // 2))
    sphere += np.array([[0.1], [0.1], [0.2]])
    slab = lo[:, None] - 0.1 + (hi - lo + 0.2)[:, None] * rng.random((3, n - n // 2))
    slab[2] = 0.3 + 0.02 * rng.standard_normal(n - n // 2)
    points = np.ascontiguousarray(np.hstack([sphere, slab])[:, rng.permutation(n)])
    min_dist = 0.05
    out = dict(points=points, bbox=bbox, mask=mask, min_dist=np.float64(min_dist))
    out["voxel_mask_points"] = metrics.VoxelMask(bbox, mask).filter(points.copy())
    for tag, seed in (("", 7), ("2", 8)):
        np.random.seed(seed)
        out["reduce_density_points" + tag] = metrics.ReduceDensity(min_dist).filter(points.copy())
        np.random.seed(seed)
        order = np.arange(n)
        np.random.shuffle(order)
        out["order" + tag] = order.astype(np.int64)
        out["shuffle_seed" + tag] = np.int64(seed)
    np.savez_compressed(os.path.join(HERE, "ref_filters.npz"), **out)
    for k, v in sorted(out.items()):
        print(k, getattr(v, "shape", v), getattr(v, "dtype", ""))
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
