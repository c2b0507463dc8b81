"""tests/volume_truth.py against closed forms (CPU): the restatement the GPU tests of the
occupancy volume compare with, on grids whose rendering can be written down.  The voxel lists
are the C oracle's traversal of the fixture's segments."""
import numpy as np
import pytest

import volume_truth as vt

F = np.float32
U = 2.0 ** -24          # unit round-off of fp32


@pytest.fixture(scope="module")
def lists(oracle_mod):
    o = oracle_mod.Oracle(M=40, D=2, N=2, F=1, H=1, W=1, padding=0, bbox=vt.BBOX,
                          grid_shape=vt.GRID)
    starts, ends = vt.make_segments()
    rvi, rvc = o.traversal(starts, ends)
    vg = oracle_mod.voxel_grid_centers(vt.BBOX, vt.GRID)
    return rvi, rvc, vg


def _distance64(voxel, vg):
    return float(np.sqrt(((vg[tuple(voxel)].astype(np.float64) - np.array(vt.CENTER)) ** 2).sum()))


def _power32(base32, k):
    """base^k as the sequential fp32 product T <- T * base from T = 1"""
    T = F(1)
    for _ in range(k):
        T = F(T * base32)
    return T


def test_fixture_is_what_the_tests_need(lists):
    rvi, rvc, _ = lists
    assert len(rvc) == 197 and (rvc == 0).sum() >= 30
    assert rvc.max() < 40 and rvc[rvc > 0].min() == 1 and rvc.max() >= 20


def test_belief64_is_the_clamped_logistic():
    a = np.array([0.0, 2.0, -2.0, 9.2, -9.2, 9.3, -9.3, 40.0, -40.0, -200.0], F)
    b = vt.belief64(a)
    assert b.dtype == np.float64
    assert b[0] == 0.5 and abs(b[1] - 1 / (1 + np.exp(-2.0))) < 1e-15 and abs(b[1] + b[2] - 1) < 1e-15
    assert vt.LO < b[4] < b[3] < vt.HI                   # |9.2| is inside the clamp
    assert b[5] == b[7] == vt.HI and b[6] == b[8] == b[9] == vt.LO
    assert vt.HI == float(F(1 - 1e-4))


def test_voxel_distance_is_the_fp32_distance(lists):
    rvi, rvc, vg = lists
    rows = np.where(rvc > 0)[0]
    t = vt.voxel_distance32(rvi[rows, 0], vg, vt.CENTER)
    assert t.dtype == F
    want = np.array([_distance64(rvi[r, 0], vg) for r in rows])
    # differences, squares, two additions, a square root: 3.5 u relative at the most
    assert np.abs(t - want).max() <= 4 * U * want.max()


def test_uniform_floor_grid(lists):
    """1e-4 everywhere: w decreases strictly, so the first voxel is the depth; the ray never
    loses half of its light; opacity is 1 - (1 - 1e-4)^c."""
    rvi, rvc, vg = lists
    belief = np.full(vt.GRID, 1e-4, F)
    out = vt.render32(rvi, rvc, belief, vg, vt.CENTER)
    assert out.shape == (5, len(rvc)) and out.dtype == F
    keep = F(F(1) - F(1e-4))
    for r in range(len(rvc)):
        c = int(rvc[r])
        if c == 0:
            assert not out[:, r].any()
            continue
        t0 = vt.voxel_distance32(rvi[r, 0], vg, vt.CENTER)
        assert out[0, r] == t0 and abs(float(t0) - _distance64(rvi[r, 0], vg)) <= 4 * U * 5
        assert out[1, r] == F(F(1) - _power32(keep, c))
        assert abs(float(out[1, r]) - (1 - (1 - 1e-4) ** c)) <= (c + 2) * U
        assert out[3, r] == F(1e-4) and out[4, r] == 0
        # every t of the list bounds the weighted mean
        ts = vt.voxel_distance32(rvi[r, :c], vg, vt.CENTER)
        assert ts.min() * (1 - 1e-5) <= out[2, r] <= ts.max() * (1 + 1e-5)


def test_one_wall(lists):
    """1e-4 but for a wall of 1 - 1e-4 at x = 9, first met at list index k: depth and median
    are t_k, the confidence (1 - 1e-4)^(k + 1)."""
    rvi, rvc, vg = lists
    belief = np.full(vt.GRID, 1e-4, F)
    belief[9] = F(1 - 1e-4)
    out = vt.render32(rvi, rvc, belief, vg, vt.CENTER)
    keep = F(F(1) - F(1e-4))
    seen = 0
    for r in range(len(rvc)):
        c = int(rvc[r])
        hits = np.where(rvi[r, :c, 0] == 9)[0]
        if c == 0:
            assert not out[:, r].any()
        if len(hits) == 0:
            continue
        k = int(hits[0])
        seen += 1
        tk = vt.voxel_distance32(rvi[r, k], vg, vt.CENTER)
        assert out[0, r] == tk and out[4, r] == tk
        conf = F(F(1 - 1e-4) * _power32(keep, k))
        assert out[3, r] == conf
        assert abs(float(conf) - (1 - 1e-4) ** (k + 1)) <= (k + 3) * U
        assert out[1, r] >= 1 - 1.01e-4          # T behind the wall is at most 1 - fl32(1 - 1e-4)
    assert seen >= 60


def test_rows_without_voxels_are_zero(lists):
    rvi, rvc, vg = lists
    rng = np.random.default_rng(3)
    belief = rng.uniform(1e-4, 1 - 1e-4, vt.GRID).astype(F)
    # (whatever the unused list entries hold)
    out = vt.render32(np.where(rvc[:, None, None] == 0, 5, rvi), rvc, belief, vg, vt.CENTER)
    assert (rvc == 0).sum() >= 30 and not out[:, rvc == 0].any()
    assert np.isfinite(out).all() and (out[1] >= 0).all() and (out[1] <= 1).all()
