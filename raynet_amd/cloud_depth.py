"""Ground-truth depth maps from a point cloud: the cloud's z-buffer in every view, on the GPU.

The DTU dataset ships the ground truth of a scan as one point cloud (Points/stl/stlNNN_total.ply);
the z-depth maps `DTUScene` reads (Depth/scanNNN/*.npy) are made from it.  `CloudDepthRenderer`
keeps the cloud on the device and renders it into any number of views with one kernel launch
(include/raynet_hip.h, rn_cloud_zbuffer):

  * raw z-buffer: a point's projection is formed in float64, every operation rounded on its own;
    it lands on the pixel (rint(u), rint(v)) (half to even) and the pixel keeps the smallest
    fp32 camera-space z of the points that land on it, +inf where none does -- exact and
    independent of the points' order, bit for bit np.minimum.at on the same inputs;
  * hidden-point filter: points of back surfaces show through the gaps between the points of a
    front surface.  A pixel keeps its depth iff it is within a slope-dependent tolerance of the
    smallest depth of its (2S+1)^2 window; fp32, elementwise, torch ops on the device
    (`hidden_point_filter`, restated operation for operation in tests/cloud_truth.py).

The map is only as good as the cloud is dense: below about one point per pixel footprint more
and more pixels stay empty.

There is no CPU route: without a GPU the constructor raises RaynetHipError.
"""
import numpy as np
import torch

from . import _lib

EMPTY_BITS = 0x7F800000         # +inf as a float bit pattern: the fill value of the raw buffer
MAX_POINTS_PER_LAUNCH = 1 << 30


def camera_rows(cameras):
    """[V, 21] float64: K (3x3), R (3x3), t (3) of every camera, row-major, widened from
    whatever dtype the camera holds."""
    rows = np.empty((len(cameras), 21), dtype=np.float64)
    for k, cam in enumerate(cameras):
        rows[k, 0:9] = np.asarray(cam.K, dtype=np.float64).reshape(9)
        rows[k, 9:18] = np.asarray(cam.R, dtype=np.float64).reshape(9)
        rows[k, 18:21] = np.asarray(cam.t, dtype=np.float64).reshape(3)
    return rows


def filter_coefficients(rows, closing_radius, slope_gain, tau_px):
    """The filter's two fp32 coefficients, formed in float64 on the host and rounded once:
    (slope_gain * closing_radius, [V] tau_px / K_00)."""
    ks = np.float32(float(slope_gain) * int(closing_radius))
    tf = (float(tau_px) / np.asarray(rows, dtype=np.float64)[:, 0]).astype(np.float32)
    return ks, tf


def hidden_point_filter(z0, ks, tf, closing_radius):
    """Kept mask [V, H, W] (bool) of the raw buffers z0 [V, H, W] f32 (+inf = empty); ks, tf:
    `filter_coefficients`.  Every step is one fp32 operation per element, in this order:

        zc  = min of z0 over the (2S+1)^2 window, +inf outside the image
        gx  = (zc[x+1] - zc[x-1]) * 0.5 where both are finite (and inside), else 0; gy likewise
        thr = (zc + ks * (|gx| + |gy|)) + zc * tf
        keep = z0 <= thr   (what an empty pixel, z0 = +inf, gets here is never used)
    """
    S = int(closing_radius)
    V, H, W = z0.shape
    zc = -torch.nn.functional.max_pool2d(-z0.unsqueeze(1), 2 * S + 1, stride=1,
                                         padding=S).squeeze(1)

    def central(lo, hi):
        d = (hi - lo) * 0.5
        return torch.where(torch.isfinite(lo) & torch.isfinite(hi), d, torch.zeros_like(d))

    gx = torch.zeros_like(zc)
    gy = torch.zeros_like(zc)
    if W > 2:
        gx[:, :, 1:-1] = central(zc[:, :, :-2], zc[:, :, 2:])
    if H > 2:
        gy[:, 1:-1, :] = central(zc[:, :-2, :], zc[:, 2:, :])
    slope = (gx.abs() + gy.abs()) * torch.tensor(ks, dtype=torch.float32, device=z0.device)
    tol = zc * torch.from_numpy(np.asarray(tf, np.float32)).to(z0.device).view(V, 1, 1)
    return z0 <= (zc + slope) + tol


class CloudDepthRenderer(object):
    """A point cloud [n, 3] (float32; host array or tensor) kept on the device, rendered into
    z-depth maps of `raynet_amd.common.camera.Camera` views."""

    def __init__(self, points, device=None):
        if not torch.cuda.is_available():
            raise _lib.RaynetHipError(
                "no GPU visible: raynet_amd renders point clouds on MI355X only (no CPU fallback)")
        from .hip_implementations import get_context
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else int(device))
        if isinstance(points, torch.Tensor):
            pts = points.detach().to(device=self.device, dtype=torch.float32)
        else:
            pts = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(self.device)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError("points: expected [n, 3], got %s" % (tuple(pts.shape),))
        self.points = pts.contiguous()
        self.n_points = int(pts.shape[0])
        with torch.cuda.device(self.device):
            self._ctx = get_context()

    def _rows(self, cameras, H, W):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError("H, W: at least 1, got %d, %d" % (H, W))
        return camera_rows(cameras), H, W

    def zbuffer_bits(self, rows, H, W, counts=None):
        """The raw buffers as float bit patterns, [V, H, W] int32 (device), for camera rows
        [V, 21] f64; counts: None or a zeroed [2] int64 device tensor (landed pairs | atomics
        the pre-test skipped)."""
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64)).to(self.device)
        zbuf = torch.full((rows.shape[0], H, W), EMPTY_BITS, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            # one launch takes 2^30 points; a larger cloud accumulates chunk by chunk
            for a in range(0, self.n_points, MAX_POINTS_PER_LAUNCH):
                self._ctx.cloud_zbuffer(self.points[a:a + MAX_POINTS_PER_LAUNCH], rows, H, W, zbuf,
                                        counts)
        return zbuf

    def zbuffer(self, cameras, H, W):
        """[V, H, W] f32 device tensor: per view and pixel the smallest camera-space z of the
        points that project onto it, +inf where none does."""
        rows, H, W = self._rows(cameras, H, W)
        return self.zbuffer_bits(rows, H, W).view(torch.float32)

    def depth_maps(self, cameras, H, W, closing_radius=1, slope_gain=1.5, tau_px=1.0):
        """[V, H, W] f32 device tensor of z-depth maps, 0 where a pixel is empty or its point is
        hidden behind a nearer surface (the layout of DTU's Depth/scanNNN/*.npy).
        closing_radius = 0 switches the hidden-point filter off."""
        S = int(closing_radius)
        if S < 0:
            raise ValueError("closing_radius: >= 0, got %d" % S)
        if not (float(slope_gain) >= 0.0 and float(tau_px) >= 0.0):
            raise ValueError("slope_gain, tau_px: >= 0, got %r, %r" % (slope_gain, tau_px))
        rows, H, W = self._rows(cameras, H, W)
        z0 = self.zbuffer_bits(rows, H, W).view(torch.float32)
        keep = torch.isfinite(z0)
        if S > 0 and z0.numel():
            ks, tf = filter_coefficients(rows, S, slope_gain, tau_px)
            keep &= hidden_point_filter(z0, ks, tf, S)
        return torch.where(keep, z0, torch.zeros_like(z0))
