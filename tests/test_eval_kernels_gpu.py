"""The evaluation kernels of csrc/raynet_eval.inl (k_depth_points, k_consistency_tau, k_nn) on
the GPU against their NumPy restatements (tests/eval_truth.py), bit for bit, at the sizes and
values where they can go wrong: image shapes that are no multiple of the block, degenerate depths,
projections that end in .5 or are not numbers, reference clouds around the LDS tile, equal
distances, non-finite rows -- and the argument checks of the three HipContext wrappers, which
raise before anything is launched.

"Bit for bit" is eval_truth.same_bits: NaN where the truth has NaN, every other element the same
bits."""
import numpy as np
import pytest
import torch

import eval_truth as truth

pytestmark = pytest.mark.gpu

SENTINEL = 123.25


def _ctx():
    from raynet_amd.hip_implementations import get_context
    return get_context()


def _cuda(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _host(t):
    return t.cpu().numpy()


# ---- back-projection ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,w", [(5, 7, 1.0), (7, 5, 1.0), (1, 300, 1.0), (300, 1, 1.0),
                                   (17, 31, 1.0), (17, 31, 0.75)])
def test_depth_points_bits(H, W, w):
    """Every pixel has its own depth (a transposed read cannot pass), among them 0, a negative
    one and +inf; 17 * 31 = 527 and 300 are no multiples of the block; center[3] != 1 pins the
    fourth component of the norm.  Nothing is written behind the 3 * H * W doubles."""
    rng = np.random.default_rng(1000 * H + W)
    P_pinv = rng.standard_normal((4, 3))
    assert np.linalg.matrix_rank(P_pinv) == 3
    center = np.append(rng.uniform(-1.0, 1.0, 3), w)
    n = H * W
    depth = (1.0 + 0.25 * rng.permutation(n)).astype(np.float32)
    depth[[3, n // 2, n - 2]] = [0.0, -2.5, np.inf]
    assert len(np.unique(depth)) == n
    depth = depth.reshape(H, W)
    want = truth.depth_points(H, W, P_pinv, center, depth)
    if w != 1.0:
        assert not truth.same_bits(want, truth.depth_points(H, W, P_pinv, np.append(center[:3], 1.0), depth))
    buf = torch.full((3 * n + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    _ctx().depthmap_points(H, W, _cuda(P_pinv), _cuda(center), _cuda(depth), buf)
    got = _host(buf)
    assert np.all(got[3 * n:] == SENTINEL)
    got = got[:3 * n].reshape(3, n)
    # depth 0 gives the centre itself, +inf a point at infinity
    zero = (3 % W) * H + 3 // W
    assert np.array_equal(want[:, zero], center[:3])
    assert np.isinf(want).any() and not np.isnan(want).any()
    assert truth.same_bits(got, want), "%d of %d values differ" % (
        np.sum(got.view(np.uint64) != want.view(np.uint64)), want.size)


# ---- consistency -------------------------------------------------------------------------------
CH, CW = 6, 9
# view 1 has integer entries: a point (x, y, 1) projects to exactly (x + 0.5, y + 1.5)
C_P = [np.array([[0.8, 0, 0.6, -0.028], [0, 0.8, 0.9, 0.098], [0, 0, 1.0, 0.02]]),
       np.array([[2.0, 0, 1, 0], [0, 2.0, 3, 0], [0, 0, 2.0, 0]]),
       np.array([[2.0, 0, 1, -2], [0, 2.0, 1, 2], [0, 0, 1.0, 1]])]
C_CENTER = [np.array([0.05, -0.1, -0.02, 1.0]), np.array([0.0, 0, 0, 1]),
            np.array([1.5, -0.5, -1.0, 1.0])]


def _consistency_scene():
    """(points (3, n), depth maps [3] (CH, CW) f32 with NaN pixels, number of hand-placed points).
    The hand-placed points come first, so the first n points hold them for every n but 1."""
    rng = np.random.default_rng(11)
    hand = [(0.0, 0.0, 0.0),                 # h2 == 0, h0 == 0: NaN
            (1.0, 0.5, 0.0),                 # h2 == 0, h0 != 0: inf
            (1e300, 0.5, 1.0)]               # 1e300
    hand += [(k, 0.5, 1.0) for k in range(-1, CW)]          # x: -0.5, 0.5, ... W - 0.5
    hand += [(0.5, k - 1.0, 1.0) for k in range(-1, CH)]    # y: -0.5, 0.5, ... H - 0.5
    hand = np.array(hand).T
    qx, qy = truth.projection(hand, C_P[1])
    assert np.isnan(qx[0]) and np.isinf(qx[1]) and qx[2] == 1e300
    assert qx[3:3 + CW + 1].tolist() == [k + 0.5 for k in range(-1, CW)]       # even and odd k
    assert qy[3 + CW + 1:].tolist() == [k + 0.5 for k in range(-1, CH)]
    assert np.all(qy[3:3 + CW + 1] == 2.0) and np.all(qx[3 + CW + 1:] == 1.0)
    P0_pinv = np.linalg.pinv(C_P[0])
    layers = [truth.depth_points(CH, CW, P0_pinv, C_CENTER[0],
                                 (t + 0.1 * rng.random((CH, CW))).astype(np.float32))
              for t in np.linspace(0.5, 3.0, 11)]
    points = np.hstack([hand] + layers)
    depths = []
    for v in range(3):
        d = (0.5 + 0.125 * rng.permutation(CH * CW)).astype(np.float32).reshape(CH, CW)
        d.ravel()[rng.choice(CH * CW, 9, replace=False)] = np.nan
        depths.append(d)
    depths[1][0, 0] = 2.0        # where a wrongly "valid" NaN projection would read a number
    depths[1][2, 1] = np.nan     # hand-placed points land here: NaN that later views must keep
    return points, depths, hand.shape[1]


@pytest.fixture(scope="module")
def cscene():
    return _consistency_scene()


@pytest.mark.parametrize("order", [(0, 1, 2), (1, 2, 0), (2, 0, 1)])
@pytest.mark.parametrize("n", [1, 255, 257, None])
def test_consistency_tau_bits(cscene, n, order):
    """Three calls (first = 1, 0, 0) over the views in `order`, tau compared after every call.
    View 1 is the one the hand-placed points leave or do not project into at all: it comes second,
    first and last.  tau has one element more than points; it keeps its value.

    While the kernel converted rint(h0 / h2) to int before the range test, the point (0, 0, 0),
    whose projection into view 1 is NaN, came back from a first call on view 1 as 2.0 =
    |depth[0][0] - 0| instead of inf (the conversion of NaN gives 0 on this hardware); in the
    other two orders an earlier or later view the point is outside of hid it."""
    points, depths, n_hand = cscene
    n = points.shape[1] if n is None else n
    assert points.shape[1] > 600 and (n == 1 or n > n_hand)
    pts = np.ascontiguousarray(points[:, :n])
    ctx = _ctx()
    d_pts = _cuda(pts)
    tau = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    tau[n] = SENTINEL
    want = None
    seen = dict(nan_kept=0, inf_after_number=0, inf_kept=0)
    for k, v in enumerate(order):
        before = want
        want = truth.consistency_tau(pts, C_P[v], C_CENTER[v], depths[v], before, k == 0)
        ctx.consistency_tau(CH, CW, k == 0, d_pts, _cuda(C_P[v]), _cuda(C_CENTER[v]),
                            _cuda(depths[v]), tau)
        got = _host(tau)
        assert got[n] == SENTINEL
        bad = np.nonzero(~((got[:n] == want) | (np.isnan(got[:n]) & np.isnan(want))))[0]
        assert truth.same_bits(got[:n], want), "view %d (call %d): points %s: got %s, truth %s" % (
            v, k, bad[:8], got[:n][bad[:8]], want[bad[:8]])
        if before is not None:
            seen["nan_kept"] += int(np.sum(np.isnan(before) & np.isnan(want)))
            seen["inf_after_number"] += int(np.sum(np.isfinite(before) & np.isinf(want)))
            seen["inf_kept"] += int(np.sum(np.isinf(before) & np.isinf(want)))
    assert np.isinf(want[0])                         # the NaN projection, whichever view came when
    if n > 1:
        # (a later view that the point does project into, onto a NaN pixel, turns inf into NaN)
        assert not np.isfinite(want[:3]).any(), want[:3]
        assert min(seen.values()) > 0, seen          # the orderings do exercise the three rules


def test_consistency_hand_points_cover_both_edges(cscene):
    """The premise of the .5 cases, on the truth alone: in view 1, -0.5 rounds to -0 (inside),
    W - 0.5 = 8.5 to 8 (inside), 7.5 to 8, H - 0.5 = 5.5 to 6 (outside)."""
    points, depths, n_hand = cscene
    tau = truth.consistency_tau(points[:, :n_hand], C_P[1], C_CENTER[1],
                                np.ones((CH, CW), np.float32), None, True)
    inside_x = np.isfinite(tau[3:3 + CW + 1])
    inside_y = np.isfinite(tau[3 + CW + 1:])
    assert inside_x.all()                            # -0.5 -> 0 ... 7.5 -> 8, 8.5 -> 8
    assert inside_y.tolist() == [True] * CH + [False]        # 4.5 -> 4, 5.5 -> 6 = H


# ---- nearest neighbours ------------------------------------------------------------------------
NN_PAIRS = [(1, 1), (1, 257), (1, 511), (63, 255), (63, 256), (63, 512), (2047, 256), (2047, 513),
            (2047, 1025), (2048, 1), (2048, 511), (2048, 1025), (2049, 257), (2049, 512),
            (2049, 513), (4101, 255), (4101, 513), (4101, 1025)]


def _nn(ref, qry, want_dist=True, want_idx=True, pad=3):
    """Run the scan; outputs have `pad` more elements than queries, which must keep their value."""
    nq = qry.shape[0]
    dist = torch.full((nq + pad,), SENTINEL, dtype=torch.float32, device="cuda") if want_dist else None
    idx = torch.full((nq + pad,), -77, dtype=torch.int32, device="cuda") if want_idx else None
    _ctx().nearest_neighbors(ref if isinstance(ref, torch.Tensor) else _cuda(ref),
                             qry if isinstance(qry, torch.Tensor) else _cuda(qry), dist, idx)
    out = []
    if want_dist:
        d = _host(dist)
        assert np.all(d[nq:] == SENTINEL)
        out.append(d[:nq])
    if want_idx:
        i = _host(idx)
        assert np.all(i[nq:] == -77)
        out.append(i[:nq])
    return out


def _assert_nn_equals_truth(ref, qry):
    want_d, want_i = truth.nearest(ref, qry)
    got_d, got_i = _nn(ref, qry)
    assert got_i.dtype == np.int32 and np.array_equal(got_i, want_i), "%d indices differ" % np.sum(
        got_i != want_i)
    assert truth.same_bits(got_d, want_d)
    return want_d, want_i


@pytest.mark.parametrize("n_ref,n_query", NN_PAIRS)
def test_nn_lattice_with_ties(n_ref, n_query):
    """Integer reference points in 0..5, queries on the half-integer lattice: distances tie in
    their bits and the lowest index must win -- across LDS tiles too."""
    ref, qry = truth.lattice_cloud(n_ref, n_query, seed=n_ref + n_query)
    want_d, want_i = _assert_nn_equals_truth(ref, qry)
    if n_ref >= 2047:
        d2 = truth.squared_distances(ref, qry)
        tied = d2 == d2.min(axis=1, keepdims=True)
        assert np.mean(tied.sum(axis=1) >= 2) > 0.5
        if n_ref == 4101:
            tile = np.arange(n_ref) // truth.NN_TILE
            later = (tied & (tile[None, :] > tile[want_i][:, None])).any(axis=1)
            assert np.mean(later) > 0.5


@pytest.mark.parametrize("n_ref,n_query", NN_PAIRS)
def test_nn_at_dtu_scale(n_ref, n_query):
    ref, qry = truth.dtu_cloud(n_ref, n_query, seed=n_ref + n_query)
    _assert_nn_equals_truth(ref, qry)


def test_nn_ignores_the_w_lane_and_rows_behind_the_clouds():
    ref, qry = truth.lattice_cloud(2049, 513, seed=5)
    plain_d, plain_i = _nn(ref, qry)
    ref_buf = np.full((2049 + 7, 4), 1e30, np.float32)
    qry_buf = np.full((513 + 7, 4), 1e30, np.float32)
    ref_buf[:2049], qry_buf[:513] = ref, qry
    ref_buf[:2049, 3] = np.nan
    qry_buf[:513, 3] = np.nan
    got_d, got_i = _nn(_cuda(ref_buf)[:2049], _cuda(qry_buf)[:513])
    assert np.array_equal(got_i, plain_i) and truth.same_bits(got_d, plain_d)
    want_d, want_i = truth.nearest(ref_buf[:2049], qry_buf[:513])
    assert np.array_equal(got_i, want_i) and truth.same_bits(got_d, want_d)


def test_nn_single_outputs_and_empty_calls():
    from raynet_amd._lib import RaynetHipError
    ref, qry = truth.dtu_cloud(2049, 513, seed=6)
    both_d, both_i = _nn(ref, qry)
    (only_d,) = _nn(ref, qry, want_idx=False)
    (only_i,) = _nn(ref, qry, want_dist=False)
    assert truth.same_bits(only_d, both_d) and np.array_equal(only_i, both_i)
    ctx = _ctx()
    d_ref, d_qry = _cuda(ref), _cuda(qry)
    with pytest.raises(ValueError):
        ctx.nearest_neighbors(d_ref, d_qry, None, None)
    dist = torch.full((513,), SENTINEL, dtype=torch.float32, device="cuda")
    idx = torch.full((513,), -77, dtype=torch.int32, device="cuda")
    with pytest.raises((ValueError, RaynetHipError)):
        ctx.nearest_neighbors(d_ref[:0], d_qry, dist, idx)
    ctx.nearest_neighbors(d_ref, d_qry[:0], dist, idx)          # n_query = 0: nothing to do
    torch.cuda.synchronize()
    assert np.all(_host(dist) == SENTINEL) and np.all(_host(idx) == -77)


def test_nn_non_finite_rows_and_queries():
    ref, qry = truth.dtu_cloud(2049, 513, seed=7)
    clean_d, clean_i = truth.nearest(ref, qry)
    # the rows most queries would choose: NaN and inf in their place
    chosen = np.bincount(clean_i, minlength=2049).argsort()[-2:]
    ref[chosen[0], :3] = np.nan
    ref[chosen[1], :3] = [np.inf, 500.0, -np.inf]
    qry[[0, 300, 512], :3] = [[np.nan, 500, 500], [500, np.inf, 500], [500, 500, np.nan]]
    want_d, want_i = _assert_nn_equals_truth(ref, qry)
    assert not np.isin(want_i, chosen).any()
    assert want_i[[0, 300, 512]].tolist() == [-1, -1, -1] and np.all(np.isinf(want_d[[0, 300, 512]]))
    assert np.all(want_i[1:300] >= 0) and np.all(np.isfinite(want_d[1:300]))
    # nothing to choose from
    for n_ref in (1, 2049):
        got_d, got_i = _nn(np.full((n_ref, 4), np.nan, np.float32), qry)
        assert np.all(got_i == -1) and np.all(np.isposinf(got_d))


class _EveryOther(object):
    """A filter as metrics.VoxelMask / ReduceDensity are: .filter(points) -> the kept columns,
    a new array."""

    def filter(self, points):
        return np.ascontiguousarray(points[:, ::2])


def test_pointcloud_index_follows_filter():
    """Pointcloud.index() keeps the device copy of the points until the cloud changes:
    Pointcloud.filter() changes it."""
    from raynet_amd.pointcloud import Pointcloud
    ref, _ = truth.dtu_cloud(1001, 1, seed=8)
    X = np.ascontiguousarray(ref[:, :3].T)                      # (3, N) float32
    cloud = Pointcloud(X)
    d, i = cloud.nearest_neighbors(X)
    assert np.all(d == 0) and np.array_equal(i.ravel(), np.arange(1001))
    cloud.filter(_EveryOther())
    assert cloud.points.shape == (3, 501)
    d, i = cloud.nearest_neighbors(X)
    want_d, want_i = truth.nearest(truth.xyzw(X[:, ::2].T), truth.xyzw(X.T))
    assert d.shape == (1001, 1) and np.array_equal(i.ravel(), want_i)
    assert truth.same_bits(d.ravel().astype(np.float32), want_d)
    assert np.all(d[1::2] > 0) and np.all(d[::2] == 0)


# ---- the wrappers refuse what the kernels would read out of bounds ---------------------------
def _raises_and_leaves(call, *outputs):
    """ValueError, and no output changed (nothing was launched)."""
    before = [o.clone() for o in outputs]
    with pytest.raises(ValueError):
        call()
    torch.cuda.synchronize()
    for o, b in zip(outputs, before):
        assert torch.equal(o, b)


def test_depthmap_points_rejects_bad_arguments():
    ctx = _ctx()
    H, W = 5, 7
    P = _cuda(np.random.default_rng(0).standard_normal((4, 3)))
    c = _cuda(np.array([0.1, 0.2, 0.3, 1.0]))
    depth = torch.ones((H, W), dtype=torch.float32, device="cuda")
    pts = torch.full((3, H * W), SENTINEL, dtype=torch.float64, device="cuda")
    ctx.depthmap_points(H, W, P, c, depth, pts.clone())                  # the good call
    for bad in (lambda: ctx.depthmap_points(H, W, P.float(), c, depth, pts),     # wrong dtypes
                lambda: ctx.depthmap_points(H, W, P, c, depth.double(), pts),
                lambda: ctx.depthmap_points(H, W, P, c, depth, pts.float()),
                lambda: ctx.depthmap_points(H, W, P, c[:3], depth, pts),         # 3-element centre
                lambda: ctx.depthmap_points(H, W, P[:3], c, depth, pts),         # short matrix
                lambda: ctx.depthmap_points(H, W + 1, P, c, depth, pts),         # short map
                lambda: ctx.depthmap_points(H, W, P, c, depth, pts[:, :-1]),     # strided, short
                lambda: ctx.depthmap_points(H, W, P, c, depth.t(), pts),         # strided view
                lambda: ctx.depthmap_points(0, W, P, c, depth, pts),
                lambda: ctx.depthmap_points(H, W, P.cpu(), c, depth, pts)):
        _raises_and_leaves(bad, pts)


def test_consistency_tau_rejects_bad_arguments():
    ctx = _ctx()
    H, W, n = 5, 7, 40
    P = _cuda(np.array([[2.0, 0, 1, 0], [0, 2.0, 3, 0], [0, 0, 2.0, 0]]))
    c = _cuda(np.array([0.0, 0, 0, 1]))
    depth = torch.ones((H, W), dtype=torch.float32, device="cuda")
    pts = torch.ones((3, n), dtype=torch.float64, device="cuda")
    tau = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    ctx.consistency_tau(H, W, True, pts, P, c, depth, tau.clone())       # the good call
    wide = torch.ones((3, 2 * n), dtype=torch.float64, device="cuda")
    for bad in (lambda: ctx.consistency_tau(H, W, True, pts.float(), P, c, depth, tau),
                lambda: ctx.consistency_tau(H, W, True, pts, P, c, depth, tau.float()),
                lambda: ctx.consistency_tau(H, W, True, pts, P, c, depth.double(), tau),
                lambda: ctx.consistency_tau(H, W, True, pts, P, c[:3], depth, tau),      # centre
                lambda: ctx.consistency_tau(H, W, True, pts, P, c, depth, tau[:n - 1]),  # short tau
                lambda: ctx.consistency_tau(H, W, True, wide[:, ::2], P, c, depth, tau),  # strided
                lambda: ctx.consistency_tau(H, W, True, pts.t().contiguous(), P, c, depth, tau),
                lambda: ctx.consistency_tau(H, W, True, pts.reshape(-1), P, c, depth, tau),
                lambda: ctx.consistency_tau(H, W, True, pts, P[:2], c, depth, tau),
                lambda: ctx.consistency_tau(H + 3, W, True, pts, P, c, depth, tau)):
        _raises_and_leaves(bad, tau)


def test_nearest_neighbors_rejects_bad_arguments():
    ctx = _ctx()
    ref, qry = truth.lattice_cloud(100, 40)
    d_ref, d_qry = _cuda(ref), _cuda(qry)
    dist = torch.full((40,), SENTINEL, dtype=torch.float32, device="cuda")
    idx = torch.full((40,), -77, dtype=torch.int32, device="cuda")
    ctx.nearest_neighbors(d_ref, d_qry, dist.clone(), idx.clone())       # the good call
    planar = torch.zeros((3, 100), dtype=torch.float32, device="cuda")
    wide = torch.zeros((200, 4), dtype=torch.float32, device="cuda")
    for bad in (lambda: ctx.nearest_neighbors(d_ref.double(), d_qry, dist, idx),     # float64 cloud
                lambda: ctx.nearest_neighbors(d_ref, d_qry.double(), dist, idx),
                lambda: ctx.nearest_neighbors(planar, d_qry, dist, idx),             # (3, n)
                lambda: ctx.nearest_neighbors(d_ref, planar, dist, idx),
                lambda: ctx.nearest_neighbors(d_ref[:, :3], d_qry, dist, idx),       # (n, 3) view
                lambda: ctx.nearest_neighbors(wide[::2], d_qry, dist, idx),          # strided rows
                lambda: ctx.nearest_neighbors(d_ref.reshape(-1)[1:-3].reshape(-1, 4), d_qry, dist, idx),
                lambda: ctx.nearest_neighbors(d_ref, d_qry, dist[:39], idx),         # short outputs
                lambda: ctx.nearest_neighbors(d_ref, d_qry, dist, idx[:39]),
                lambda: ctx.nearest_neighbors(d_ref, d_qry, idx, dist),              # swapped dtypes
                lambda: ctx.nearest_neighbors(d_ref, d_qry, None, None),
                lambda: ctx.nearest_neighbors(ref, d_qry, dist, idx)):               # host array
        _raises_and_leaves(bad, dist, idx)
