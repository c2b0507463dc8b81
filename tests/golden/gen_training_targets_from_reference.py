#!/usr/bin/env python3
"""Golden target distributions of the pre-training stage: dirac_distribution and
gaussian_distribution (raynet/utils/training_utils.py:71-141) for both `std_is_distance` values,
produced by the reference's own functions (lib2to3 scratch copy under /tmp, see
gen_pointcloud_from_reference.py for the loader) on sample points and ground-truth points of
valid rays of the mock Restrepo plane scene (tests/batch_truth.py).  Arrays only.
Output: ref_training_targets.npz."""
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_pointcloud_from_reference import REF, load_reference   # noqa: E402

STDDEV_FACTORS = (1.0, 2.5)


def main():
    import batch_truth as bt
    _, _, _, scratch = load_reference()
    pkg = os.path.join(scratch, "refpc")
    shutil.copy(os.path.join(REF, "raynet", "utils", "training_utils.py"),
                os.path.join(pkg, "utils", "training_utils.py"))
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n",
                           os.path.join(pkg, "utils", "training_utils.py")],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    tu = importlib.import_module("refpc.utils.training_utils")

    scene = bt.plane_scene(HERE)
    N, D = 5, 32
    cams, nbr = bt.tables(scene, N)
    rng = np.random.default_rng(11)
    view = rng.integers(0, bt.VIEWS, 400).astype(np.int32)
    ridx = rng.integers(0, bt.H * bt.W, 400).astype(np.int32)
    depth = np.array([scene.get_depth_map(v)[r % bt.H, r // bt.H] for v, r in zip(view, ridx)],
                     np.float32)
    t = bt.batch_rays_f32(view, ridx, depth, cams, nbr, np.asarray(scene.bbox, np.float32).ravel(),
                          bt.H, bt.W, D, (11, 11))
    keep = np.nonzero(t["flags"] == 0)[0][:96]
    points, targets = t["points"][keep], t["target"][keep]
    out = {"points": points, "targets": targets,
           "stddev_factors": np.array(STDDEV_FACTORS, np.float32)}
    out["dirac"] = np.stack([tu.dirac_distribution(tg.reshape(4, 1), p)
                             for tg, p in zip(targets, points)])
    for flag in (False, True):
        for f in STDDEV_FACTORS:
            fn = tu.gaussian_distribution(f, flag)
            out["gaussian_%s_%g" % ("distance" if flag else "squared", f)] = np.stack(
                [fn(tg.reshape(4, 1), p) for tg, p in zip(targets, points)])
    np.savez_compressed(os.path.join(HERE, "ref_training_targets.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})
    shutil.rmtree(scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
