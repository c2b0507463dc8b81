"""On-disk Restrepo datasets for the training tests: scenes of the mock cameras looking at the
plane z = 0.3 (tests/batch_truth.py), written the way the loaders read them -- imgs/*.png,
cams_krt/*.txt (the intrinsics scaled to the image size), scene_info.xml, gt/gt_depth_%d.npy."""
import os
import shutil

import numpy as np

import batch_truth as bt


def write_plane_scene(path, golden, H=bt.H, W=bt.W, views=bt.VIEWS, depth=True):
    from PIL import Image
    scene = bt.plane_scene(golden, H=H, W=W, views=views)
    for d in ("imgs", "cams_krt", "gt"):
        os.makedirs(os.path.join(path, d))
    shutil.copy(os.path.join(golden, "restrepo_mock_scene_1", "scene_info.xml"),
                os.path.join(path, "scene_info.xml"))
    for i in range(views):
        im = scene.get_image(i)
        Image.fromarray(np.round(im.image * 255).astype(np.uint8)).save(
            os.path.join(path, "imgs", "frame_%03d.png" % i))
        cam = im.camera
        with open(os.path.join(path, "cams_krt", "frame_%03d.txt" % i), "w") as f:
            for row in np.asarray(cam.K, np.float64):
                f.write(" ".join("%.9g" % v for v in row) + "\n")
            f.write("\n")
            for row in np.asarray(cam.R, np.float64):
                f.write(" ".join("%.9g" % v for v in row) + "\n")
            f.write("\n" + " ".join("%.9g" % v for v in np.asarray(cam.t, np.float64).ravel()) + "\n")
        if depth:
            np.save(os.path.join(path, "gt", "gt_depth_%d.npy" % i), scene.get_depth_map(i))
    return scene


def write_dataset(root, golden, names=("scene_a", "scene_b"), **kw):
    """A dataset directory of plane scenes and its split file: the first scenes train, the last
    one tests.  Returns (directory, split file)."""
    import json
    directory = os.path.join(root, "dataset")
    for name in names:
        write_plane_scene(os.path.join(directory, name), golden, **kw)
    split = os.path.join(root, "split.json")
    with open(split, "w") as f:
        json.dump({"train": list(range(len(names) - 1)), "test": [len(names) - 1]}, f)
    return directory, split
