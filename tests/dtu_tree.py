"""A small scan in the DTU layout, written from known cameras (helper of the cloud-depth tests)."""
import os

import numpy as np


def write_dtu_tree(base, cameras, H, W, scan=1, points=None, depth_maps=None):
    """Rectified/scanNNN/rect_00k_max.png (H x W), cal18/intrinsic.txt and pos_00k.txt from
    `cameras` (which share one K), ObsMask<scan>_10.mat, and optionally
    Points/stl/stlNNN_total.ply from `points` [n, 3] and Depth/scanNNN/depth_00k.npy from
    `depth_maps`.  Returns base."""
    from PIL import Image as PILImage
    from scipy.io import savemat
    base = str(base)
    cal = os.path.join(base, "SampleSet/MVS_Data/Calibration/cal18")
    rect = os.path.join(base, "Rectified/scan%03d" % scan)
    for d in (cal, rect, os.path.join(base, "SampleSet/MVS_Data/ObsMask")):
        os.makedirs(d)
    K = np.asarray(cameras[0].K, np.float64)
    np.savetxt(os.path.join(cal, "intrinsic.txt"), K)
    for k, cam in enumerate(cameras):
        np.savetxt(os.path.join(cal, "pos_%03d.txt" % (k + 1)), K.dot(np.hstack([cam.R, cam.t])))
        PILImage.fromarray(np.full((H, W, 3), 40 * (k + 1), np.uint8)).save(
            os.path.join(rect, "rect_%03d_max.png" % (k + 1)))
    savemat(os.path.join(base, "SampleSet/MVS_Data/ObsMask", "ObsMask%d_10.mat" % scan),
            {"BB": np.array([[-5.0, -5.0, -1.0], [5.0, 5.0, 2.0]]), "ObsMask": np.ones((2, 2, 2))})
    if points is not None:
        os.makedirs(os.path.join(base, "Points/stl"))
        pts = np.ascontiguousarray(points, dtype="<f4").reshape(-1, 3)
        with open(os.path.join(base, "Points/stl", "stl%03d_total.ply" % scan), "wb") as f:
            f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
                     "property float y\nproperty float z\nend_header\n" % len(pts)).encode())
            pts.tofile(f)
    if depth_maps is not None:
        os.makedirs(os.path.join(base, "Depth/scan%03d" % scan))
        for k, z in enumerate(depth_maps):
            np.save(os.path.join(base, "Depth/scan%03d" % scan, "depth_%03d.npy" % (k + 1)),
                    np.asarray(z, np.float32))
    return base
