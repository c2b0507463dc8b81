"""The restatements of the evaluation kernels (tests/eval_truth.py) are
sound: held to the float64 oracle of the reference's modules (oracle/pointcloud_oracle.py) and to
the reference's own outputs (tests/golden/ref_pointcloud.npz).  No GPU."""
import os

import numpy as np
import pytest

import eval_truth as truth
from conftest import GOLDEN
from oracle import pointcloud_oracle as po

EPS64 = 2.0 ** -52
EPS32 = 2.0 ** -24          # half an ulp of float32: the relative error of one rounding


def random_camera(rng):
    """A pinhole camera with a random rotation, within 0.1 of the world's origin: (P [3][4],
    P_pinv [4][3], centre [4] with centre[3] == 1).  Its points, centre + depth * direction with
    depths of 2 to 6, have a norm within 0.2 of their depth: the norm is the size of every term
    that is rounded, which is what makes "ulp of the point's norm" a measure of rounding (a
    camera that looks AT the origin cancels centre against depth * direction, and no rounding
    error is small against a norm near 0)."""
    f = rng.uniform(20.0, 40.0)
    K = np.array([[f, 0.0, rng.uniform(2.0, 6.0)], [0.0, f, rng.uniform(2.0, 6.0)], [0.0, 0.0, 1.0]])
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(R) < 0:
        R[:, 0] = -R[:, 0]
    C = rng.uniform(-0.1, 0.1, 3)
    P = K.dot(np.hstack([R, -R.dot(C).reshape(3, 1)]))
    return P, np.linalg.pinv(P), np.append(C, 1.0)


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "ref_pointcloud.npz"))


@pytest.mark.parametrize("shape", [(5, 7), (1, 9), (9, 1)])
def test_depth_points_equals_the_oracle(shape):
    """The oracle takes its rays from a matrix product and sums the norm in NumPy's order; the
    truth follows the kernel.  Same definition, so a last-bit difference in a ray or in the norm
    is all that can separate them: within 4 ulp of the point's norm (see random_camera)."""
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    for _ in range(4):
        _, P_pinv, center = random_camera(rng)
        depth = rng.uniform(2.0, 6.0, (H, W)).astype(np.float32)
        ones = np.ones((H, W), np.float32)
        got = truth.depth_points(H, W, P_pinv, center, depth)
        assert got.shape == (3, H * W) and got.dtype == np.float64
        sel = po.selected_pixels(ones, 0)[0]
        assert np.array_equal(np.sort(sel), np.arange(H * W))
        want = po.points_per_image(P_pinv, center, depth, ones, 0)
        assert np.all(want[3] == 1.0)
        err = np.abs(got[:, sel] - want[:3]).max(axis=0)
        norm = np.linalg.norm(want[:3], axis=0)
        print("depth_points %s: max error %.3g ulp of the norm" % (shape, (err / (EPS64 * norm)).max()))
        assert np.all(err <= 4 * EPS64 * norm)


def _golden_frame_points(g, i):
    H, W = int(g["H"]), int(g["W"])
    pts = truth.depth_points(H, W, g["P_pinv"][i], g["center"][i], po.clean_depth(g["pred"][i]))
    return pts[:, po.selected_pixels(g["gt"][i], int(g["borders"]))[0]]


def test_depth_points_reproduces_the_golden_cloud(g):
    assert np.isnan(g["pred"]).any()                # the NaN replacement is exercised
    pts = np.hstack([_golden_frame_points(g, i) for i in range(len(g["P"]))])
    assert pts.shape == g["points_plain"].shape
    assert np.abs(pts - g["points_plain"]).max() < 1e-9


def test_consistency_tau_reproduces_the_surviving_set(g):
    n_views = len(g["P"])
    neigh = po.camera_neighbors(list(g["center"]), int(g["n_neighbors"]))
    kept = []
    for f in range(n_views):
        pts = _golden_frame_points(g, f)
        tau = None
        for k, i in enumerate(neigh[f]):
            tau = truth.consistency_tau(pts, g["P"][i], g["center"][i], g["pred"][i], tau, k == 0)
        kept.append(pts[:, tau < float(g["consistency_threshold"])])
    kept = np.hstack(kept)
    assert kept.shape == g["points_consistency"].shape        # the same points survive
    assert np.abs(kept - g["points_consistency"]).max() < 1e-9


def _assert_nearest_within_roundings(ref, qry):
    """d2 = (dx*dx + dy*dy) + dz*dz on the same float32 inputs: three roundings on the longest
    path into a term (difference, square, one or two sums), the square doubling the first --
    at most 5 roundings on d2, halved by the root, plus the root's own: 3.5 < 4 roundings."""
    dist, idx = truth.nearest(ref, qry)
    assert dist.dtype == np.float32 and idx.dtype == np.int32
    want = po.nearest_distances(ref[:, :3].T, qry[:, :3].T)
    rel = np.abs(dist.astype(np.float64) - want) / want
    print("nearest: max relative error %.3g" % rel.max())
    assert np.all(rel <= 4 * EPS32)
    return dist, idx


def test_nearest_at_unit_scale_equals_the_float64_oracle():
    rng = np.random.default_rng(3)
    ref = truth.xyzw(rng.standard_normal((3001, 3)))
    qry = truth.xyzw(rng.standard_normal((1000, 3)))
    dist, idx = _assert_nearest_within_roundings(ref, qry)
    assert idx.min() >= 0 and idx.max() < 3001
    # a point of the cloud is its own neighbour, the first of its copies
    d0, i0 = truth.nearest(np.vstack([ref, ref[:5]]), ref[:20])
    assert np.all(d0 == 0) and np.array_equal(i0, np.arange(20))


def test_nearest_at_dtu_scale_equals_the_float64_oracle():
    """Hundreds of units, neighbours 0.2 apart: the differences of nearby float32 numbers are
    exact, so the scan on the float32-rounded cloud is as good as in float64."""
    ref, qry = truth.dtu_cloud(4101, 1025)
    assert ref[:, :3].min() >= 300 and ref[:, :3].max() <= 700
    dist, idx = _assert_nearest_within_roundings(ref, qry)
    assert np.abs(dist - 0.2).max() < 1e-3
    d2 = ((qry[:, None, :3].astype(np.float64) - ref[None, :, :3]) ** 2).sum(axis=2)
    assert np.array_equal(idx, d2.argmin(axis=1))


def test_nearest_never_chooses_a_non_finite_row():
    ref = truth.xyzw([[0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3, 0, 0]], w=np.nan)
    qry = truth.xyzw([[2.9, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [1e30, 0, 0]], w=np.nan)
    dist, idx = truth.nearest(ref, qry)
    # 1e30 squared overflows float32: inf is not below inf
    assert idx.tolist() == [3, -1, -1, -1] and np.all(np.isinf(dist[1:]))
    assert dist[0] == np.sqrt(np.float32(np.float32(2.9) - np.float32(3)) ** 2)
    dist, idx = truth.nearest(truth.xyzw(np.full((5, 3), np.nan)), qry)
    assert idx.tolist() == [-1] * 4 and np.all(np.isinf(dist))
    dist, idx = truth.nearest(np.zeros((0, 4), np.float32), qry)
    assert idx.tolist() == [-1] * 4 and np.all(np.isinf(dist))


def test_invalid_projections_give_inf():
    """h0 / h2 of NaN, +inf, -inf and 1e300: the reference casts np.round of them to int32, gets a
    negative number and calls the point invalid; the truth decides on the doubles."""
    P = np.hstack([np.eye(3), np.zeros((3, 1))])
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [1e300, 0, 1], [2.0, 1, 1]]).T
    qx, _ = truth.projection(pts, P)
    assert np.isnan(qx[0]) and qx[1] == np.inf and qx[2] == -np.inf and qx[3] == 1e300
    with np.errstate(invalid="ignore"):
        assert np.all(np.round(qx[:4]).astype(np.int32) < 0)        # the reference's route
    depth = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    center = np.array([0.0, 0, 0, 1])
    for first in (True, False):
        tau = truth.consistency_tau(pts, P, center, depth, np.zeros(5), first)
        assert np.all(tau[:4] == np.inf)
        assert tau[4] == abs(float(depth[1, 2]) - np.sqrt(6.0))


def test_consistency_tau_rounds_half_to_even_and_orders_nan_and_inf():
    P = np.array([[2.0, 0, 1, 0], [0, 2.0, 3, 0], [0, 0, 2.0, 0]])     # (x + 0.5, y + 1.5) at z = 1
    xs = np.array([-1.0, 0.0, 1.0, 2.0, 2.5, 3.0])
    pts = np.stack([xs, np.zeros(6), np.ones(6)])
    qx, qy = truth.projection(pts, P)
    assert qx.tolist() == [-0.5, 0.5, 1.5, 2.5, 3.0, 3.5] and np.all(qy == 1.5)
    W = 4
    depth = np.arange(12, dtype=np.float32).reshape(3, W)
    center = np.array([0.0, 0, 0, 1])
    dist = np.sqrt(xs * xs + 1.0)
    tau = truth.consistency_tau(pts, P, center, depth, None, True)
    # -0.5 -> -0 (valid, column 0), 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3 -> 3, 3.5 -> 4 = W: outside
    cols = [0, 0, 2, 2, 3]
    assert np.array_equal(tau[:5], np.abs(depth[2, cols].astype(np.float64) - dist[:5]))
    assert tau[5] == np.inf
    # NaN depth: NaN now, NaN after a valid view, inf after an invalid one, inf stays inf
    nan_map = np.full((3, W), np.nan, np.float32)
    t1 = truth.consistency_tau(pts, P, center, nan_map, None, True)
    assert np.all(np.isnan(t1[:5])) and t1[5] == np.inf
    t2 = truth.consistency_tau(pts, P, center, depth, t1, False)
    assert np.all(np.isnan(t2[:5])) and t2[5] == np.inf
    P_out = P.copy()
    P_out[0, 3] = 100.0                               # every point lands right of the image
    t3 = truth.consistency_tau(pts, P_out, center, depth, t2, False)
    assert np.all(t3 == np.inf)
    t4 = truth.consistency_tau(pts, P, center, depth, t3, False)
    assert np.all(t4 == np.inf)
    # `first` does not read tau_in
    assert truth.same_bits(truth.consistency_tau(pts, P, center, depth, t3, True), tau)
