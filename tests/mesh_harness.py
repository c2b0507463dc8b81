"""What the GPU tests of the mesh stages share (plain functions, imported like the *_truth.py
restatements): the context and the upload, outputs and workspaces that are longer than asked for
and prefilled, the assertions that nothing behind the used part was written and that an input kept
its bits, the bit-for-bit comparison with its message, the scene directory the chain tests hand to
the command line, and the depth maps of the two spheres those chains start from."""
import os

import numpy as np

F = np.float32
D = np.float64
PAD = 5                 # rows behind every output
TAIL = 64               # bytes behind the workspace
TAIL_BYTE = 0xA5


def ctx():
    from raynet_amd.hip_implementations import get_context
    return get_context()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def cuda(a, dtype=None):
    """The array as a contiguous device tensor of the given numpy dtype (None stays None)."""
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _rows(a):
    return a.reshape(len(a), int(np.prod(a.shape[1:])))


# ------------------------------------------------------------------------------ the guard rows
def padded(shape, fill, dtype, pad=PAD, device="cuda"):
    """An output of shape[0] + pad rows, every element prefilled."""
    import torch
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    return torch.full((shape[0] + pad,) + shape[1:], fill, dtype=dtype, device=device)


def workspace(need, tail=TAIL, device="cuda"):
    """A workspace of need + tail bytes of 0xA5."""
    import torch
    return torch.full((need + tail,), TAIL_BYTE, dtype=torch.uint8, device=device)


def assert_untouched(buffer, used, fill, what=""):
    """Rows [used:] of a prefilled tensor or array (bytes, for a workspace) still hold the
    prefill's bits."""
    a = np.ascontiguousarray(_host(buffer)[used:])
    raw = _rows(a.view("u%d" % a.itemsize))
    written = (raw != np.array(fill, a.dtype).view(raw.dtype)).any(1)
    assert not written.any(), (what, "written behind row %d" % used,
                               (used + np.flatnonzero(written))[:5])


def assert_input_kept(tensor, uploaded, what=""):
    """A device input has the bits it was uploaded with."""
    after = _host(tensor)
    before = np.ascontiguousarray(uploaded, after.dtype).reshape(after.shape)
    assert np.array_equal(after.view("u%d" % after.itemsize),
                          before.view("u%d" % after.itemsize)), (what, "an input was written")


def assert_same_bits(got, want, what="", nan_payloads=False):
    """float32 rows equal bit for bit; the message names how many differ, the first five of them
    and the first three rows of both.  With nan_payloads a NaN matches any NaN (a NaN that an
    operation makes -- inf - inf -- has the sign and payload of the machine that made it, which
    no definition fixes): NaN where the truth has NaN, and the bits everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = bits(got) != bits(want)
    if nan_payloads:
        differ &= ~(np.isnan(got) & np.isnan(want))
    differ = _rows(differ).any(1)
    assert not differ.any(), (what, int(differ.sum()), np.flatnonzero(differ)[:5],
                              got[differ][:3], want[differ][:3])


# ------------------------------------------------------------------------------ the chain's scene
def write_restrepo_scene(path, bbox, cameras, H, W, gt_maps):
    """A Restrepo scene directory of the given box, cameras (as text) and ground-truth depth
    maps, with grey images."""
    from PIL import Image as PILImage
    for d in ("imgs", "cams_krt", "gt"):
        os.makedirs(os.path.join(path, d))
    with open(os.path.join(path, "scene_info.xml"), "w") as f:
        f.write('<?xml version="1.0" encoding="UTF-8" standalone="yes"?>\n<bwm_info_for_boxm2>\n'
                '  <bbox minx="%.9g" miny="%.9g" minz="%.9g" maxx="%.9g" maxy="%.9g" maxz="%.9g">\n'
                '  </bbox>\n</bwm_info_for_boxm2>\n' % tuple(float(b) for b in bbox))
    for i, (cam, depth) in enumerate(zip(cameras, gt_maps)):
        PILImage.fromarray(np.full((H, W, 3), 40 * i + 60, np.uint8)).save(
            os.path.join(path, "imgs", "frame_%03d.png" % i))
        with open(os.path.join(path, "cams_krt", "frame_%03d.txt" % i), "w") as f:
            for row in np.asarray(cam.K, D):
                f.write(" ".join("%.9g" % x for x in row) + "\n")
            f.write("\n")
            for row in np.asarray(cam.R, D):
                f.write(" ".join("%.9g" % x for x in row) + "\n")
            f.write("\n" + " ".join("%.9g" % x for x in np.asarray(cam.t, D).ravel()) + "\n")
        np.save(os.path.join(path, "gt", "gt_depth_%d.npy" % i), depth)


NOISE_SIGMA, NOISE_SEED = 0.02, 0       # chosen on the CPU with the restatements: DESIGN.md 23
PATCH = (slice(9, 11), slice(14, 16))   # blanked in every view: chosen on the CPU with the truths


def two_sphere_maps(noise_sigma=None, seed=NOISE_SEED, blank=None):
    """The scene of the chain tests: the box [-1, 1]^3, three cameras on a
    ring, a large sphere and a small one whose surfaces are 0.36 apart, a grid of 18 x 22 x 14
    -> (bbox, cameras, H, W, grid, big, small, gt_maps).  The maps are the nearer sphere's depth,
    0 where a ray meets neither; with noise_sigma, normal noise on the pixels that see a sphere;
    with blank, that patch of every view (which saw a sphere) set to 0 afterwards."""
    import fusion_truth as ft
    from raynet_amd.synthetic import ring_cameras
    H, W, grid = 20, 30, (18, 22, 14)
    bbox = np.array([-1, -1, -1, 1, 1, 1], F)
    big, small = ((0.0, 0.0, -0.1), 0.5), ((-0.6, 0.55, 0.5), 0.15)
    cams = ring_cameras(3, H, W, focal=1.5 * H)
    rng = np.random.default_rng(seed)
    gt_maps = []
    for cam in cams:
        d = np.minimum(ft.sphere_depth(cam, H, W, *big), ft.sphere_depth(cam, H, W, *small))
        d = np.where(np.isfinite(d), d, F(0)).astype(F)
        if noise_sigma is not None:
            d = np.where(d > 0, d + rng.normal(scale=noise_sigma, size=d.shape).astype(F),
                         F(0)).astype(F)
        if blank is not None:
            assert (d[blank] > 0).all()
            d[blank] = 0
        gt_maps.append(d)
    return bbox, cams, H, W, grid, big, small, gt_maps
