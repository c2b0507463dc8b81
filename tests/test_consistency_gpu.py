"""The cross-view check on the GPU: rn_points_consistency against
tests/consistency_truth.py -- the three masks as uint32 and the residual as its bits, every entry,
no tolerance -- over the sizes at which a launch can go wrong, 1 to 32 views, inputs planted on
every branch of the definition, the entries behind the outputs, the entry's refusals, the package's
check_depth_maps (which undoes rn_depthmap_points' column order) and the chain from filtered maps
to a fused volume."""
import ctypes

import numpy as np
import pytest

import consistency_truth as ct
import eval_truth as et
import fusion_truth as ft
from appearance_truth import PlaneCamera, pack_cameras
from mesh_harness import PAD, assert_untouched, cuda

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
MASK_FILL, RESIDUAL_FILL = -7, -7.0
TOLERANCES = [(0.08, 0.0), (0.0, 0.025), (0.03, 0.01)]


def _ctx():
    from raynet_amd.hip_implementations import get_context
    return get_context()


def _run(points, cameras, depths, exclude, tol_abs, tol_rel, border, uploaded=None):
    """rn_points_consistency on points [3, n] with outputs PAD entries longer than n and prefilled
    -> (seen, agree, violate u32 [n], residual f32 [n]) after checking that the PAD entries kept
    their prefill.  uploaded: the device (cameras, depths) of an earlier call with the same
    ones."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = _ctx()
    points = np.ascontiguousarray(points, D).reshape(3, -1)
    n = points.shape[1]
    V, H, W = depths.shape
    d_cameras, d_depths = uploaded or (cuda(cameras, D), cuda(depths, F))
    d_points = cuda(points)
    masks = [torch.full((n + PAD,), MASK_FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    residual = torch.full((n + PAD,), RESIDUAL_FILL, dtype=torch.float32, device="cuda")
    ctx._check(ctx.lib.rn_points_consistency(
        ctx._h, n, _ptr(d_points), V, _ptr(d_cameras), H, W, _ptr(d_depths), int(exclude),
        float(tol_abs), float(tol_rel), float(border), _ptr(masks[0]), _ptr(masks[1]),
        _ptr(masks[2]), _ptr(residual), _stream()))
    for m in masks:
        assert_untouched(m, n, np.int32(MASK_FILL), "a mask")
    assert_untouched(residual, n, F(RESIDUAL_FILL), "residual")
    return tuple(m.cpu().numpy()[:n].view(np.uint32) for m in masks) + (residual.cpu().numpy()[:n],)


def _same(got, want, what):
    for name, g, w in zip(("seen", "agree", "violate"), got[:3], want[:3]):
        assert g.dtype == w.dtype == np.uint32 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.flatnonzero(g != w)[:5])
    g, w = got[3], want[3]
    assert g.dtype == w.dtype == F and np.isfinite(g).all(), what
    differ = g.view(np.uint32) != w.view(np.uint32)
    assert not differ.any(), (what, "residual", int(differ.sum()), np.flatnonzero(differ)[:5],
                              g[differ][:3], w[differ][:3])


def _held_to_the_truth(points, cameras, depths, exclude, tol_abs, tol_rel, border, what,
                       uploaded=None):
    want = ct.check_points(points, cameras, depths, exclude, tol_abs, tol_rel, border)
    got = _run(points, cameras, depths, exclude, tol_abs, tol_rel, border, uploaded)
    _same(got, want, (what, exclude, tol_abs, tol_rel, border))
    return want


# ------------------------------------------------------------------------------ a. the plane
@pytest.fixture(scope="module")
def plane():
    cams, rows, depths, kind = ct.perturbed_plane_scene()
    return dict(cams=cams, rows=rows, depths=depths, kind=kind,
                points=ct.back_project(cams[0], depths[0]))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 527, 768])
def test_the_masks_and_the_residual_are_the_restatement_bit_for_bit(plane, n):
    """V = 3 on the plane scene with its floater and dent: the first n pixels' points (all 768:
    24 x 32), a NaN and two infinite points among them from n = 63 on; every view excluded in turn
    and none; each tolerance alone and both; border 0 and 2.5."""
    points = plane["points"][:, :n].copy()
    if n >= 63:
        points[0, 5], points[1, 17], points[2, 40] = np.nan, np.inf, -np.inf
    rows, depths = plane["rows"], plane["depths"]
    uploaded = (cuda(rows, D), cuda(depths, F))
    bits = 0
    for exclude in (0, -1, 1, 2):
        for tol_abs, tol_rel in TOLERANCES:
            for border in (0.0, 2.5):
                want = _held_to_the_truth(points, rows, depths, exclude, tol_abs, tol_rel, border,
                                          "plane, n %d" % n, uploaded)
                bits += int(ct.popcount(want[0]).sum())
                if n >= 63:
                    for k in (5, 17, 40):
                        assert want[0][k] == want[1][k] == want[2][k] == 0 and want[3][k] == 0
    print("n %d: %d seen bits over the 24 settings" % (n, bits))
    assert bits > 0
    if n == 768:
        seen, agree, violate, _ = ct.check_points(points, rows, depths, 0, 0.08, 0.0, 0.0)
        kind = plane["kind"].reshape(-1)
        assert violate[kind == 1].all() and not violate[kind != 1].any()    # the scene decides


# ------------------------------------------------------------------------------ b. the views
def _ring(V, H, W):
    """V cameras over the plane z = 0 at slightly different centres, and their analytic maps."""
    cams = [PlaneCamera(0.3 * np.cos(0.7 * v), 0.3 * np.sin(0.7 * v), 3.0 + 0.01 * v, 20.0,
                        (W - 1) / 2.0, (H - 1) / 2.0) for v in range(V)]
    Y, X = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    depths = []
    for cam in cams:
        gx, gy = cam.ground_point(X, Y)
        depths.append(np.sqrt((gx - cam.cx) ** 2 + (gy - cam.cy) ** 2 + cam.height ** 2).astype(F))
    return cams, np.stack(depths)


@pytest.mark.parametrize("V", [1, 2, 32])
def test_one_two_and_thirty_two_views(V):
    """V = 1 with the only view excluded sets nothing; V = 2; V = 32 with only views 0 and 31
    measuring anything (the others hold 0, negative, NaN and +inf): bit 31 is set and compared."""
    H, W = 13, 17
    cams, depths = _ring(V, H, W)
    rows = pack_cameras(cams)
    if V == 32:
        for v in range(1, 31):
            depths[v] = (0.0, -1.0, np.nan, np.inf)[v % 4]
    points = ct.back_project(cams[0], (depths[0] * F(1.01)).astype(F))
    for exclude in sorted({-1, 0, V - 1}):
        for tol_abs, tol_rel in TOLERANCES:
            want = _held_to_the_truth(points, rows, depths, exclude, tol_abs, tol_rel, 0.0,
                                      "V %d" % V)
            if V == 1 and exclude == 0:
                assert not any(w.any() for w in want)
            if V == 32:
                assert not (want[0] & np.uint32(0x7FFFFFFE)).any()
                if exclude != 31:
                    assert (want[0] & np.uint32(0x80000000)).any()
                    assert ((want[1] | want[2]) & np.uint32(0x80000000)).any()
                else:
                    assert not (want[0] & np.uint32(0x80000000)).any()


# ------------------------------------------------------------------------------ c. planted
def _planted():
    """View 0 (and view 1, the same camera over another map) looks straight down from (0, 0, 4)
    with focal 16 and principal point (8, 8): a point (x, y, z) lands at (16 x / (4 - z) + 8,
    16 y / (4 - z) + 8), exactly for the dyadic numbers used here."""
    H, W = 24, 32
    cam = PlaneCamera(0.0, 0.0, 4.0, 16.0, 8.0, 8.0)
    rows = pack_cameras([cam, cam])
    rng = np.random.default_rng(11)
    depths = rng.uniform(3.0, 6.0, (2, H, W)).astype(F)
    depths[0, 8, 8] = 2.0                                   # zm = 2 under the points of the band
    depths[0, 8, 10:14] = np.array([0, -1, np.nan, np.inf], F)
    names, pts = [], []

    def plant(name, p):
        names.append(name)
        pts.append(p)

    plant("s = 0.75: zm 2, dd 1", (0, 0, 3))
    plant("s = -1.25: zm 2, dd 9", (0, 0, 1))
    plant("behind the camera", (0, 0, 5))
    plant("on the camera plane", (1, 0, 4))
    plant("at the centre", (0, 0, 4))
    plant("NaN", (np.nan, 0, 0))
    plant("inf", (0, np.inf, 0))
    plant("-inf", (0, 0, -np.inf))
    for k, name in enumerate(("depth 0", "depth negative", "depth NaN", "depth inf")):
        plant(name, ((10 + k - 8) / 4.0, 0, 0))
    # halves in both parities, along x and along y: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    for half in (0.5, 1.5, 2.5, 3.5):
        plant("X = %g" % half, ((half - 8) / 4.0, 0.25, 0))
        plant("Y = %g" % half, (0.25, (half - 8) / 4.0, 0))
    # on the border, for border 0 and 2.5, and one fp64 step outside
    for X in (0.0, 31.0, 2.5, 28.5):
        plant("border X = %g" % X, ((X - 8) / 4.0, 0.5, 0))
    for Y in (0.0, 23.0, 2.5, 20.5):
        plant("border Y = %g" % Y, (0.5, (Y - 8) / 4.0, 0))
    plant("X just below 0", (np.nextafter(-2.0, -np.inf), 0.5, 0))
    plant("X just above W - 1", (np.nextafter(5.75, np.inf), 0.5, 0))
    return dict(H=H, W=W, rows=rows, depths=depths, names=names, points=np.array(pts, D).T.copy())


def test_planted_inputs_decide_every_branch():
    p = _planted()
    rows, depths, points, names = p["rows"], p["depths"], p["points"], p["names"]
    at_ = {name: k for k, name in enumerate(names)}
    uploaded = (cuda(rows, D), cuda(depths, F))
    below = lambda x: float(np.nextafter(x, 0.0))           # noqa: E731
    settings = [(0.75, 0.0), (below(0.75), 0.0), (1.25, 0.0), (below(1.25), 0.0), (0.0, 0.375),
                (0.0, below(0.375)), (0.0, 0.625), (0.0, below(0.625)), (0.25, 0.25), (0.25, 0.5),
                (0.0, 0.0), (3.0, 0.0), (0.0, 1.0)]
    got = {}
    for border in (0.0, 2.5):
        for exclude in (-1, 1):
            for tol_abs, tol_rel in settings:
                got[(border, exclude, tol_abs, tol_rel)] = _held_to_the_truth(
                    points, rows, depths, exclude, tol_abs, tol_rel, border, "planted", uploaded)

    def view0(name, tol_abs, tol_rel, border=0.0):
        seen, agree, violate, residual = got[(border, 1, tol_abs, tol_rel)]
        k = at_[name]
        return int(seen[k] & 1), int(agree[k] & 1), int(violate[k] & 1), float(residual[k])

    # the bounds of the band belong to it: s == t agrees, one step less violates
    high, low = "s = 0.75: zm 2, dd 1", "s = -1.25: zm 2, dd 9"
    for t in ((0.75, 0.0), (0.0, 0.375), (0.25, 0.25)):
        assert view0(high, *t) == (1, 1, 0, 0.75), t
    for t in ((below(0.75), 0.0), (0.0, below(0.375))):
        assert view0(high, *t) == (1, 0, 1, 0.0), t
    # s == -t agrees, one step less is occluded: seen alone
    for t in ((1.25, 0.0), (0.0, 0.625), (0.25, 0.5)):
        assert view0(low, *t) == (1, 1, 0, -1.25), t
    for t in ((below(1.25), 0.0), (0.0, below(0.625))):
        assert view0(low, *t) == (1, 0, 0, 0.0), t
    # what no view measures, however wide the tolerance
    for name in ("behind the camera", "on the camera plane", "at the centre", "NaN", "inf", "-inf",
                 "depth 0", "depth negative", "depth NaN", "depth inf", "X just below 0",
                 "X just above W - 1"):
        for border in (0.0, 2.5):
            assert view0(name, 3.0, 0.0, border)[:3] == (0, 0, 0), name
    for name in ("NaN", "inf", "-inf", "behind the camera", "at the centre"):
        seen, agree, violate, residual = got[(0.0, -1, 3.0, 0.0)]
        assert seen[at_[name]] == 0 and residual[at_[name]] == 0, name
    # ... but view 1, the same camera over a map without the planted depths, measures there
    assert got[(0.0, -1, 3.0, 0.0)][0][at_["depth NaN"]] == 2
    # the border: on it is inside, for both borders
    for name in ("border X = 0", "border X = 31", "border Y = 0", "border Y = 23"):
        assert view0(name, 3.0, 0.0, 0.0)[0] == 1 and view0(name, 3.0, 0.0, 2.5)[0] == 0, name
    for name in ("border X = 2.5", "border X = 28.5", "border Y = 2.5", "border Y = 20.5"):
        assert view0(name, 3.0, 0.0, 0.0)[0] == 1 and view0(name, 3.0, 0.0, 2.5)[0] == 1, name
    # halves go to the even pixel: the residual is that pixel's, and not its odd neighbour's
    for axis in "XY":
        for half, even in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4)):
            name = "%s = %g" % (axis, half)
            k = at_[name]
            x, y = ((even, 9) if axis == "X" else (9, even))
            zm = D(depths[0, y, x])
            d = np.array([0, 0, 4.0]) - points[:, k]
            dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert view0(name, 3.0, 0.0)[3] == float(F((zm * zm - dd) / (zm + zm))), name
            other = D(depths[0, y, x + 1] if axis == "X" else depths[0, y + 1, x])
            assert F((other * other - dd) / (other + other)) != F((zm * zm - dd) / (zm + zm))


# ------------------------------------------------------------------------------ d. the wrapper
def test_check_depth_maps_undoes_the_column_order(plane):
    """check_depth_maps on the plane scene (H != W: a transpose cannot pass) equals the truth
    applied to eval_truth.depth_points' points, brought to (H, W) by indexing with u*H + v; a NaN
    depth is passed through and its pixel is never kept."""
    from raynet_amd.consistency import DepthConsistency, check_depth_maps
    cams, rows = plane["cams"], plane["rows"]
    depths = plane["depths"].copy()
    depths[1, 4, 7] = np.nan
    depths[2, 20, 3] = 0.0
    H, W = depths.shape[1:]
    pinvs, centres = zip(*[ct.pinv_and_centre(c) for c in cams])
    results = check_depth_maps(list(depths), cams, P_pinvs=pinvs, centers=centres, tol_abs=0.08,
                               tol_rel=0.0)
    assert len(results) == 3 and all(isinstance(r, DepthConsistency) for r in results)
    at_ = np.arange(W)[None, :] * H + np.arange(H)[:, None]         # pixel (v, u) -> u*H + v
    for r, c in enumerate(results):
        points = et.depth_points(H, W, pinvs[r], centres[r], depths[r])
        want = [w[at_] for w in ct.check_points(points, rows, depths, r, 0.08, 0.0, 0.0)]
        assert c.seen.shape == (H, W) and c.residual.shape == (H, W)
        _same((c.seen, c.agree, c.violate, c.residual), want, "view %d" % r)
        assert np.array_equal(c.keep(1), ct.keep(depths[r], want[1], want[2], 1))
        assert np.array_equal(c.agree_count, ct.popcount(want[1]))
        assert np.array_equal(c.filtered(depths[r], 1) != 0, ct.keep(depths[r], want[1], want[2], 1))
    # where the floater and the dent are, in the image's own coordinates
    c = results[0]
    assert (c.violate_count[ct.FLOATER] == 2).all() and (c.agree_count[ct.FLOATER] == 0).all()
    assert (c.seen_count[ct.DENT] == 2).all() and not c.violate[ct.DENT].any()
    untouched = plane["kind"] == 0
    assert not c.violate[untouched].any() and not c.keep(1)[~untouched].any()
    # the NaN pixel of view 1 and the empty one of view 2: no bit, never kept
    assert results[1].seen[4, 7] == 0 and not results[1].keep(0, 32)[4, 7]
    assert not results[2].keep(0, 32)[20, 3]
    assert results[1].filtered(depths[1], 0, 32)[4, 7] == 0


def test_check_points_takes_a_cloud(plane):
    from raynet_amd.consistency import check_points
    got = check_points(plane["points"].T, plane["cams"], list(plane["depths"]), exclude=0,
                       tol_abs=0.0, tol_rel=0.025, border=2.5)
    _same(tuple(got), ct.check_points(plane["points"], plane["rows"], plane["depths"], 0, 0.0,
                                      0.025, 2.5), "check_points")
    # float32 vertices are widened
    v = plane["points"].T.astype(F)
    got = check_points(v, plane["cams"], list(plane["depths"]))
    _same(tuple(got), ct.check_points(v.T.astype(D), plane["rows"], plane["depths"], -1, 0.0, 0.01,
                                      0.0), "check_points, float32")


# ------------------------------------------------------------------------------ e. the chain
def test_filtered_maps_fuse_and_leave_the_rest_of_the_volume_alone():
    """The sphere at 60 x 80: every map is checked against the other seven and filtered with the
    default rule; the filtered maps are the truth's, they fuse, and the volume keeps its bits at
    every voxel that reads none of the dropped pixels."""
    from raynet_amd.consistency import check_depth_maps
    from raynet_amd.fusion import fuse_depth_maps
    s = ft.sphere_scene(H=60, W=80)
    H, W, cams, rows, depths = 60, 80, s["cameras"], s["rows"], s["depths"]
    results = check_depth_maps(list(depths), cams, tol_abs=0.1, tol_rel=0.0)
    at_ = np.arange(W)[None, :] * H + np.arange(H)[:, None]
    filtered, dropped = [], []
    for r, c in enumerate(results):
        points = et.depth_points(H, W, cams[r].P_pinv, np.asarray(cams[r].center, D).reshape(4),
                                 depths[r])
        _, agree, violate, _ = [w[at_] for w in ct.check_points(points, rows, depths, r, 0.1, 0.0, 0.0)]
        keep = ct.keep(depths[r], agree, violate)
        out = c.filtered(depths[r])
        assert out.dtype == F and np.array_equal(out.view(np.uint32),
                                                 np.where(keep, depths[r], F(0)).view(np.uint32))
        filtered.append(out)
        dropped.append(np.isfinite(depths[r]) & (depths[r] > 0) & ~keep)
    n_dropped = int(sum(d.sum() for d in dropped))
    print("%d measured pixels dropped of %d" % (n_dropped, int((np.isfinite(depths)).sum())))
    assert 0 < n_dropped < np.isfinite(depths).sum()        # some go, some stay
    before = fuse_depth_maps(list(depths), cams, s["bbox"], s["grid"], trunc=s["trunc"])
    after = fuse_depth_maps(filtered, cams, s["bbox"], s["grid"], trunc=s["trunc"])
    want = ft.integrate(s["axes"], rows, np.stack(filtered), None, s["trunc"], 0.0)
    a_t, a_w = after.tsdf.cpu().numpy(), after.weight.cpu().numpy()
    assert np.array_equal(a_t.view(np.int32), want[0].view(np.int32))
    assert np.array_equal(a_w.view(np.int32), want[1].view(np.int32))
    # the voxels that read a dropped pixel in some view
    x, y, z = [g.reshape(-1) for g in np.meshgrid(*[np.asarray(a, F).astype(D) for a in s["axes"]],
                                                  indexing="ij")]
    touched = np.zeros(len(x), bool)
    with np.errstate(all="ignore"):
        for v in range(len(cams)):
            X, Y, _, _, _, _, ok = ft.project_points(rows[v], x, y, z, D(0), D(W - 1), D(H - 1))
            xi = np.rint(np.where(ok, X, 0.0)).astype(np.int64)
            yi = np.rint(np.where(ok, Y, 0.0)).astype(np.int64)
            touched |= ok & dropped[v][yi, xi]
    touched = touched.reshape(s["grid"])
    b_t, b_w = before.tsdf.cpu().numpy(), before.weight.cpu().numpy()
    assert touched.any() and not touched.all()
    assert np.array_equal(a_t.view(np.int32)[~touched], b_t.view(np.int32)[~touched])
    assert np.array_equal(a_w.view(np.int32)[~touched], b_w.view(np.int32)[~touched])
    assert not np.array_equal(a_w, b_w)                       # ... and changes where it must


# ------------------------------------------------------------------------------ f. refusals
def test_bad_arguments_are_refused_before_any_launch(plane):
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = _ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    n = 65
    dpts = cuda(plane["points"][:, :n].copy())
    dcam, ddep = cuda(plane["rows"], D), cuda(plane["depths"], F)
    masks = [torch.full((n,), MASK_FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    residual = torch.full((n,), RESIDUAL_FILL, dtype=torch.float32, device="cuda")
    #       0  1           2  3           4   5   6           7  8     9     10
    good = [n, _ptr(dpts), 3, _ptr(dcam), 24, 32, _ptr(ddep), 0, 0.08, 0.01, 0.0,
            _ptr(masks[0]), _ptr(masks[1]), _ptr(masks[2]), _ptr(residual)]
    nan, inf = float("nan"), float("inf")
    bad = [(0, -1), (0, (1 << 38) + 1), (2, 0), (2, -1), (2, 33), (4, 0), (5, 0), (4, -24),
           (7, -2), (7, 3), (8, -0.08), (8, nan), (8, inf), (9, -0.01), (9, nan), (9, inf),
           (10, -1.0), (10, nan), (10, inf)] + [(k, null) for k in (1, 3, 6, 11, 12, 13, 14)]
    for at_, value in bad:
        args = list(good)
        args[at_] = value
        assert ctx.lib.rn_points_consistency(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_points_consistency" in last(ctx._h)
    torch.cuda.synchronize()
    assert all((m == MASK_FILL).all() for m in masks) and (residual == RESIDUAL_FILL).all()
    # n == 0 returns cleanly, whatever the pointers, and writes nothing
    args = [0, null, 3, null, 24, 32, null, 0, 0.08, 0.01, 0.0, null, null, null, null]
    assert ctx.lib.rn_points_consistency(ctx._h, *args, _stream()) == _lib.RN_OK
    args = list(good)
    args[0] = 0
    assert ctx.lib.rn_points_consistency(ctx._h, *args, _stream()) == _lib.RN_OK
    torch.cuda.synchronize()
    assert all((m == MASK_FILL).all() for m in masks) and (residual == RESIDUAL_FILL).all()
    none = ctx.points_consistency(torch.empty((3, 0), dtype=torch.float64, device="cuda"), dcam,
                                  ddep, 0, 0.08, 0.01, 0.0)
    assert [tuple(t.shape) for t in none] == [(0,)] * 4
    # the wrapper: the entry's name on a refusal, and tensors that are not what the kernel reads
    with pytest.raises(_lib.RaynetHipError, match="rn_points_consistency"):
        ctx.points_consistency(dpts, dcam, ddep, 0, -1.0, 0.0, 0.0)
    for kw, match in [
            (dict(points=dpts.float()), "points"), (dict(points=dpts.t().contiguous()), "points"),
            (dict(points=dpts[:, ::2]), "points"), (dict(points=dpts.cpu()), "points"),
            (dict(cameras=dcam.float()), "cameras"), (dict(cameras=dcam[:2]), "cameras"),
            (dict(depths=ddep.double()), "depths"), (dict(depths=ddep[0]), "depths"),
            (dict(depths=ddep[:, :, ::2]), "depths"),
            (dict(depths=ddep[:1].expand(33, 24, 32).contiguous()), "depths"),
            (dict(exclude=3), "exclude"), (dict(exclude=-2), "exclude"),
            (dict(seen=masks[0][:-1]), "seen"), (dict(agree=masks[1].float()), "agree"),
            (dict(violate=masks[2][::2]), "violate"), (dict(residual=residual.double()), "residual")]:
        call = dict(points=dpts, cameras=dcam, depths=ddep, exclude=0, tol_abs=0.08, tol_rel=0.01,
                    border=0.0)
        call.update(kw)
        with pytest.raises(ValueError, match=match):
            ctx.points_consistency(**call)
    torch.cuda.synchronize()
    assert all((m == MASK_FILL).all() for m in masks) and (residual == RESIDUAL_FILL).all()
    # ... and what is accepted writes all n entries of the given outputs
    out = ctx.points_consistency(dpts, dcam, ddep, 0, 0.08, 0.0, 0.0, *masks, residual)
    assert out[0] is masks[0] and out[3] is residual
    want = ct.check_points(plane["points"][:, :n], plane["rows"], plane["depths"], 0, 0.08, 0.0, 0.0)
    _same(tuple(m.cpu().numpy().view(np.uint32) for m in masks) + (residual.cpu().numpy(),), want,
          "given outputs")
