"""tests/fusion_truth.py held to properties nobody has to trust (no GPU, no library): the fused
sphere is the sphere, to a fraction of a voxel, as an open, consistently oriented surface without
the shell behind it; and the definition's edges, each planted on its own."""
import numpy as np
import pytest

import fusion_truth as ft
import isosurface_truth as it

F = np.float32
D = np.float64


@pytest.fixture(scope="module")
def sphere():
    s = ft.sphere_scene()
    s["tsdf"], s["weight"] = ft.integrate(s["axes"], s["rows"], s["depths"], None, s["trunc"], 0.0)
    return s


def test_the_fused_sphere_is_the_sphere(sphere):
    s = sphere
    assert s["trunc"] == pytest.approx(0.48) and s["side"] == pytest.approx(0.16)
    raw = ft.mesh(s["tsdf"], s["weight"], s["axes"], s["bbox"], cleaned=False)
    v, f = ft.clean(*raw)
    r = np.sqrt((v.astype(D) ** 2).sum(1))
    off = np.abs(r - 1.0) / s["side"]
    E, two, repeated, boundary = it.edge_census(f)
    tri = v.astype(D)[f.astype(np.int64)]
    normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    outward = ((normal * tri.mean(1)).sum(1) > 0).sum()
    print("sphere: %d vertices / %d faces before cleaning, %d / %d after; distance to the sphere "
          "max %.3f mean %.3f voxel sides; %d edges, %d in two faces, %d on the boundary, %d "
          "directed edges repeated; %d of %d faces face away from the centre"
          % (len(raw[0]), len(raw[1]), len(v), len(f), off.max(), off.mean(), E, two,
             len(boundary), repeated, outward, len(f)))
    assert np.isfinite(v).all() and not np.isfinite(raw[0]).all()
    assert off.max() <= 1.0 and off.mean() <= 0.25
    assert E == two + len(boundary)                     # no edge in more than two faces
    assert repeated == 0
    assert outward >= 0.99 * len(f)
    assert len(raw[1]) / 2 < len(f) < len(raw[1])
    # cleaning keeps the order and every vertex that is left is used
    assert len(np.unique(f)) == len(v) and f.dtype == np.int32 and v.dtype == F
    kept = np.isfinite(raw[0])[raw[1]].all((1, 2))
    assert np.array_equal(raw[0][raw[1][kept]].view(np.int32), v[f].view(np.int32))


def test_every_voxel_is_written_and_finite(sphere):
    t, w = sphere["tsdf"], sphere["weight"]
    assert t.dtype == F and w.dtype == F and t.shape == sphere["grid"] == w.shape
    assert np.isfinite(t).all() and np.isfinite(w).all()
    assert (t <= 1).all() and (t >= -1).all() and (w >= 0).all() and 2 <= w.max() <= 8
    assert (w == np.rint(w)).all()                      # no weights: the number of views
    assert ((w == 0) == ((t == 1) & (w == 0))).all() and (w == 0).any()
    # min_weight masks more, never less
    a = np.isnan(ft.field(t, w, 0.0))
    b = np.isnan(ft.field(t, w, 2.0))
    assert (a <= b).all() and b.sum() > a.sum() and np.array_equal(a, w == 0)


# ------------------------------------------------------------------------------ planted cases
def _plane():
    cam = ft.PlaneCamera(0.0, 0.0, 4.0, 8.0, 4.0, 4.0)
    axes = [np.array([-0.8, -0.4, 0, 0.4, 0.8], F), np.array([-0.8, -0.4, 0, 0.4, 0.8], F),
            (0.1 + 0.25 * np.arange(9)).astype(F)]
    return cam, axes, ft.pack_cameras([cam])


def _closed_form(axes, cam_centre, z, trunc):
    x, y, zz = np.meshgrid(*[np.asarray(a, F).astype(D) for a in axes], indexing="ij")
    dx, dy, dz = cam_centre[0] - x, cam_centre[1] - y, cam_centre[2] - zz
    dd = (dx * dx + dy * dy) + dz * dz
    s = (D(z) * D(z) - dd) / (D(z) + D(z))
    return s, np.minimum(s / D(trunc), 1.0)


def test_a_plane_seen_from_above():
    cam, axes, rows = _plane()
    trunc = 0.6
    depths = np.full((1, 9, 9), 3.0, F)
    tsdf, weight = ft.integrate(axes, rows, depths, None, trunc, 0.0)
    s, t = _closed_form(axes, (0.0, 0.0, 4.0), 3.0, trunc)
    counted = s >= -trunc
    assert counted.any() and not counted.all()
    assert np.array_equal(weight, counted.astype(F))
    assert np.array_equal(tsdf.view(np.int32), np.where(counted, t, 1.0).astype(F).view(np.int32))
    # the column under the camera: unobserved behind the band, then negative, then positive up
    # to the truncation, a single zero crossing, at the plane z = 4 - 3
    col, wcol, z = tsdf[2, 2], weight[2, 2], axes[2].astype(D)
    seen = np.nonzero(wcol > 0)[0]
    assert np.array_equal(seen, np.arange(seen[0], len(z)))
    sign = np.sign(col[seen])
    assert (np.diff(sign) >= 0).all() and (np.diff(sign) > 0).sum() == 1
    below, above = z[seen][sign < 0].max(), z[seen][sign > 0].min()
    assert below < 1.0 < above and above - below == pytest.approx(0.25)
    assert col[-1] == 1.0 and wcol[-1] == 1.0           # truncated in front, but observed
    # the zero of the interpolated column is the plane to within the factor 1 - (z - r) / 2z
    k = seen[sign < 0][-1]
    zero = z[k] + (z[k + 1] - z[k]) * (0 - col[k]) / (D(col[k + 1]) - col[k])
    assert abs(zero - 1.0) <= 0.25 * trunc / (2 * 3.0)


def test_pixels_without_a_measurement_leave_their_voxels_unobserved():
    cam, axes, rows = _plane()
    depths = np.full((1, 9, 9), 3.0, F)
    planted = {(4, 6): 0.0, (4, 2): -1.0, (2, 4): np.nan, (6, 4): np.inf}
    for (py, px), value in planted.items():
        depths[0, py, px] = value
    tsdf, weight = ft.integrate(axes, rows, depths, None, 5.0, 0.0)
    plain_t, plain_w = ft.integrate(axes, rows, np.full((1, 9, 9), 3.0, F), None, 5.0, 0.0)
    assert (plain_w == 1).all()                          # trunc 5: every voxel is in the band
    x, y, z = np.meshgrid(*[a.astype(D) for a in axes], indexing="ij")
    X = np.rint(8 * x / (4 - z) + 4).astype(int)
    Y = np.rint(8 * y / (4 - z) + 4).astype(int)
    hit = np.zeros(x.shape, bool)
    for (py, px) in planted:
        here = (X == px) & (Y == py)
        assert here.any(), (py, px)
        hit |= here
    assert (weight[hit] == 0).all() and (tsdf[hit] == 1).all()
    assert np.array_equal(weight[~hit], plain_w[~hit])
    assert np.array_equal(tsdf[~hit].view(np.int32), plain_t[~hit].view(np.int32))


def _two_views():
    cams = [ft.PlaneCamera(0.0, 0.0, 4.0, 8.0, 4.0, 4.0), ft.PlaneCamera(0.3, -0.2, 3.0, 8.0, 4.0, 4.0)]
    axes = [np.array([0.1], F), np.array([-0.1], F), np.array([0.5], F)]
    depths = np.stack([np.full((9, 9), 3.4, F), np.full((9, 9), 2.7, F)])
    return cams, axes, ft.pack_cameras(cams), depths


def test_two_views_of_weights_one_and_three():
    cams, axes, rows, depths = _two_views()
    trunc = 0.7
    t = [_closed_form(axes, c.center.ravel()[:3], F(zv), trunc)[1].item()
         for c, zv in zip(cams, (3.4, 2.7))]
    assert -1 < t[0] < 1 and -1 < t[1] < 1 and t[0] != t[1]
    weights = np.stack([np.full((9, 9), 1.0, F), np.full((9, 9), 3.0, F)])
    tsdf, weight = ft.integrate(axes, rows, depths, weights, trunc, 0.0)
    assert weight.item() == 4.0
    assert tsdf.item() == F((t[0] + 3.0 * t[1]) / 4.0)
    # no weights: weight 1 each
    tsdf, weight = ft.integrate(axes, rows, depths, None, trunc, 0.0)
    assert weight.item() == 2.0 and tsdf.item() == F((t[0] + t[1]) / 2.0)


@pytest.mark.parametrize("bad", [0.0, -2.0, np.nan, np.inf])
def test_a_rejected_weight_removes_the_view(bad):
    cams, axes, rows, depths = _two_views()
    trunc = 0.7
    t0 = _closed_form(axes, cams[0].center.ravel()[:3], F(3.4), trunc)[1].item()
    weights = np.stack([np.full((9, 9), 2.0, F), np.full((9, 9), bad, F)])
    tsdf, weight = ft.integrate(axes, rows, depths, weights, trunc, 0.0)
    assert weight.item() == 2.0 and tsdf.item() == F((2.0 * t0) / 2.0)
    weights[0] = bad
    tsdf, weight = ft.integrate(axes, rows, depths, weights, trunc, 0.0)
    assert weight.item() == 0.0 and tsdf.item() == 1.0


def test_the_edge_of_the_band_counts():
    # dd = 16, z = 2: s = (4 - 16) / 4 = -3, exactly
    cam = ft.PlaneCamera(0.0, 0.0, 4.0, 8.0, 4.0, 4.0)
    axes = [np.array([0], F), np.array([0], F), np.array([0], F)]
    rows, depths = ft.pack_cameras([cam]), np.full((1, 9, 9), 2.0, F)
    tsdf, weight = ft.integrate(axes, rows, depths, None, 3.0, 0.0)
    assert weight.item() == 1.0 and tsdf.item() == -1.0
    tsdf, weight = ft.integrate(axes, rows, depths, None, np.nextafter(3.0, np.inf), 0.0)
    assert weight.item() == 1.0 and tsdf.item() == F(-3.0 / np.nextafter(3.0, np.inf))
    # one ulp: s is now below -trunc
    tsdf, weight = ft.integrate(axes, rows, depths, None, np.nextafter(3.0, 0.0), 0.0)
    assert weight.item() == 0.0 and tsdf.item() == 1.0


def test_the_border_keeps_views_off_the_edge_of_the_image():
    cam, axes, rows = _plane()
    depths = np.full((1, 9, 9), 3.0, F)
    _, w0 = ft.integrate(axes, rows, depths, None, 5.0, 0.0)
    _, w2 = ft.integrate(axes, rows, depths, None, 5.0, 2.5)
    x, y, z = np.meshgrid(*[a.astype(D) for a in axes], indexing="ij")
    X, Y = 8 * x / (4 - z) + 4, 8 * y / (4 - z) + 4
    inside = (X >= 2.5) & (X <= 5.5) & (Y >= 2.5) & (Y <= 5.5)
    assert (w0 == 1).all() and np.array_equal(w2, inside.astype(F)) and not inside.all()


def test_no_view_at_all():
    s = ft.sphere_scene(H=4, W=5, grid=(3, 4, 5), V=1)
    tsdf, weight = ft.integrate(s["axes"], np.zeros((0, 15)), np.zeros((0, 4, 5), F), None, 0.5, 0.0)
    assert tsdf.shape == (3, 4, 5) and (tsdf == 1).all() and (weight == 0).all()
    v, f = ft.mesh(tsdf, weight, s["axes"], s["bbox"])
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == F and f.dtype == np.int32


def test_the_order_of_the_views_matters_in_the_last_bit_only(sphere):
    s = sphere
    rng = np.random.default_rng(4)
    weights = rng.uniform(0.1, 3.0, size=s["depths"].shape).astype(F)
    args = (s["axes"], s["rows"], s["depths"], weights, s["trunc"], 0.0)
    V = len(s["rows"])
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    num, den = ft.integrate(*args, sums=True)
    num_p, den_p = ft.integrate(*args, order=order, sums=True)
    # it MAY differ: float64 addition is not associative ...
    assert (num != num_p).any()
    # (den does not: a sum of eight float32 weights of one magnitude is exact in float64)
    assert np.array_equal(den, den_p)
    # ... but by no more than the roundings of the V - 1 additions of either order, each at most
    # half an ulp of a partial sum that |t| <= 1 keeps within den
    bound = 2 * (V - 1) * 2.0 ** -53 * np.maximum(den, den_p)
    assert (np.abs(num - num_p) <= bound).all() and (np.abs(den - den_p) <= bound).all()
    t, w = ft.integrate(*args)
    t_p, w_p = ft.integrate(*args, order=order)
    ulps = np.abs(t.view(np.int32).astype(np.int64) - t_p.view(np.int32).astype(np.int64))
    same_sign = np.signbit(t) == np.signbit(t_p)
    print("permuted views: %d of %d tsdf values differ, by at most %d float32 ulp"
          % ((ulps != 0).sum(), t.size, ulps[same_sign].max()))
    assert ulps[same_sign].max() <= 1
    assert (np.abs(t[~same_sign]) <= 1e-15).all() and (np.abs(t_p[~same_sign]) <= 1e-15).all()
    assert np.abs(w.view(np.int32).astype(np.int64) - w_p.view(np.int32)).max() <= 1
