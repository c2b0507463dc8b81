"""NumPy restatement of DESIGN.md section 14b: the z-buffer of a point cloud and the hidden-point
filter, the truth of tests/test_cloud_truth.py and tests/test_cloud_depth_gpu.py.  Nothing here
comes from the package's kernels or its torch code: only NumPy."""
import numpy as np


def camera_rows(cameras):
    """[V, 21] float64: K | R | t of Camera objects, row-major."""
    return np.array([np.concatenate([np.asarray(c.K, np.float64).ravel(),
                                     np.asarray(c.R, np.float64).ravel(),
                                     np.asarray(c.t, np.float64).ravel()]) for c in cameras],
                    dtype=np.float64).reshape(len(cameras), 21)


def project(points, row, H, W):
    """One view: (ok [n] bool, iu [n], iv [n] int64 (valid where ok), z32 [n] float32).  points
    [n, 3] (taken as float32, widened to float64), row [21] float64.  NumPy rounds every float64
    operation on its own."""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    row = np.asarray(row, dtype=np.float64)
    K, R, t = row[0:9].reshape(3, 3), row[9:18].reshape(3, 3), row[18:21]
    with np.errstate(all="ignore"):
        Xc = [((R[j, 0] * x + R[j, 1] * y) + R[j, 2] * z) + t[j] for j in range(3)]
        h = [(K[j, 0] * Xc[0] + K[j, 1] * Xc[1]) + K[j, 2] * Xc[2] for j in range(3)]
        ru, rv = np.rint(h[0] / h[2]), np.rint(h[1] / h[2])          # half to even
        z32 = Xc[2].astype(np.float32)
        # every comparison is False for a NaN
        ok = (h[2] > 0) & (h[2] < np.inf) & (Xc[2] > 0) & (z32 < np.inf) & \
             (ru >= 0) & (ru < W) & (rv >= 0) & (rv < H)
        iu = np.where(ok, ru, 0).astype(np.int64)
        iv = np.where(ok, rv, 0).astype(np.int64)
    return ok, iu, iv, z32


def zbuffer(points, rows, H, W):
    """[V, H, W] float32, +inf where no point lands; rows [V, 21] float64."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 21)
    out = np.full((len(rows), H, W), np.inf, dtype=np.float32)
    for k, row in enumerate(rows):
        ok, iu, iv, z32 = project(points, row, H, W)
        np.minimum.at(out[k], (iv[ok], iu[ok]), z32[ok])
    return out


def landed_pairs(points, rows, H, W):
    """The number of (point, view) pairs that land on a pixel."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 21)
    return int(sum(project(points, row, H, W)[0].sum() for row in rows))


def window_min(z, S):
    """Minimum over the (2S+1)^2 window, +inf outside the image; z [V, H, W]."""
    V, H, W = z.shape
    pad = np.full((V, H + 2 * S, W + 2 * S), np.inf, dtype=z.dtype)
    pad[:, S:S + H, S:S + W] = z
    out = np.full_like(z, np.inf)
    for dy in range(2 * S + 1):
        for dx in range(2 * S + 1):
            out = np.minimum(out, pad[:, dy:dy + H, dx:dx + W])
    return out


def filter_keep(z0, rows, closing_radius=1, slope_gain=1.5, tau_px=1.0):
    """Kept mask [V, H, W] of the raw buffers z0 (float32, +inf = empty): a filled pixel stays
    iff z0 <= (zc + ks * (|gx| + |gy|)) + zc * tf, all float32, one rounding per operation;
    ks = float32(slope_gain * S) and tf = float32(tau_px / K_00) are formed in float64."""
    z0 = np.asarray(z0, dtype=np.float32)
    filled = np.isfinite(z0)
    S = int(closing_radius)
    if S == 0:
        return filled
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 21)
    ks = np.float32(float(slope_gain) * S)
    tf = (float(tau_px) / rows[:, 0]).astype(np.float32).reshape(-1, 1, 1)
    zc = window_min(z0, S)
    gx = np.zeros_like(zc)
    gy = np.zeros_like(zc)
    with np.errstate(all="ignore"):
        lo, hi = zc[:, :, :-2], zc[:, :, 2:]
        gx[:, :, 1:-1] = np.where(np.isfinite(lo) & np.isfinite(hi),
                                  (hi - lo) * np.float32(0.5), np.float32(0))
        lo, hi = zc[:, :-2, :], zc[:, 2:, :]
        gy[:, 1:-1, :] = np.where(np.isfinite(lo) & np.isfinite(hi),
                                  (hi - lo) * np.float32(0.5), np.float32(0))
        slope = (np.abs(gx) + np.abs(gy)) * ks
        thr = (zc + slope) + zc * tf
        keep = filled & (z0 <= thr)
    assert thr.dtype == np.float32
    return keep


def depth_maps(points, rows, H, W, closing_radius=1, slope_gain=1.5, tau_px=1.0):
    """[V, H, W] float32 z-depth maps, 0 where empty or hidden."""
    z0 = zbuffer(points, rows, H, W)
    keep = filter_keep(z0, rows, closing_radius, slope_gain, tau_px)
    return np.where(keep, z0, np.float32(0)).astype(np.float32)
