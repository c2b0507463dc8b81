"""Host side of the point-cloud filters: the truth code the GPU tests compare with
(tests/thin_truth.py) agrees with itself, with scikit-learn's KD-tree loop and with the
reference's own outputs (tests/golden/ref_filters.npz); the package's visiting order is the
documented hash; argument errors are raised before any device work; the coloured PLY."""
import os

import numpy as np
import pytest

import thin_truth as truth
from conftest import GOLDEN

# kept points and Jacobi rounds of the four inputs for (the seeded random order, the x-sorted
# order): regenerate with thin_truth.CASES' own seeds (DESIGN.md section 12a's table)
EXPECTED = {
    "lattice": (1728, (532, 8), (864, 34)),
    "lattice_duplicates": (1975, (550, 8), (864, 34)),
    "uniform": (6000, (1326, 8), (1489, 57)),
    "sheets": (8000, (955, 11), (1151, 133)),
}


@pytest.mark.parametrize("name", sorted(truth.CASES))
def test_the_restatements_agree(name):
    make, r, seed = truth.CASES[name]
    X = make()
    n, random_case, sorted_case = EXPECTED[name]
    assert X.shape == (3, n)
    cells = truth.cell_neighbours(X, r)
    brute = truth.brute_neighbours(X, r)
    assert all(np.array_equal(a, b) for a, b in zip(cells, brute))
    for order, (kept_count, rounds) in ((truth.random_order(n, seed), random_case),
                                        (truth.x_sorted_order(X), sorted_case)):
        kept = truth.greedy_brute(X, r, order)
        assert np.array_equal(truth.greedy_cells(X, r, order), kept)
        parallel, took = truth.parallel_rounds(X, r, order, cells)
        assert np.array_equal(parallel, kept)
        assert (int(kept.sum()), took) == (kept_count, rounds)


@pytest.mark.parametrize("name", sorted(truth.CASES))
def test_the_reference_loop_over_a_kd_tree_agrees(name):
    pytest.importorskip("sklearn.neighbors")
    make, r, seed = truth.CASES[name]
    X = make()
    for order in (truth.random_order(X.shape[1], seed), truth.x_sorted_order(X)):
        assert np.array_equal(truth.reference_loop(X, r, order), truth.greedy_cells(X, r, order))


def test_the_cells_hold_every_neighbour_off_the_lattice_and_far_from_the_origin():
    """Every neighbour of the lattice is at distance exactly r and straddles a cell border."""
    X = np.hstack([truth.lattice(), [[-0.1], [-0.07], [-0.13]]])
    for shift in (0.0, 1e6):
        Y = X + shift
        assert all(np.array_equal(a, b) for a, b in zip(truth.cell_neighbours(Y, 0.25),
                                                        truth.brute_neighbours(Y, 0.25)))


def test_the_fixture_equals_the_truth():
    z = np.load(os.path.join(GOLDEN, "ref_filters.npz"))
    X, r = z["points"], float(z["min_dist"])
    assert X.shape == (3, 3000) and X.dtype == np.float64 and z["bbox"].dtype == np.float32
    for tag in ("", "2"):
        order = z["order" + tag]
        assert np.array_equal(np.sort(order), np.arange(X.shape[1]))
        kept = truth.greedy_brute(X, r, order)
        assert np.array_equal(X[:, kept], z["reduce_density_points" + tag])
    assert not np.array_equal(z["order"], z["order2"])
    keep = truth.voxel_mask_keep(X, z["bbox"], z["mask"])
    assert np.array_equal(X[:, keep], z["voxel_mask_points"])
    assert 0 < keep.sum() < X.shape[1]


def test_the_priority_hash_is_a_permutation_and_follows_the_seed():
    from raynet_amd import metrics
    n = 5000
    orders = {}
    for seed in (0, 1, -3, 2 ** 40 + 7):
        order = truth.hash_order(seed, n)
        assert np.array_equal(np.sort(order), np.arange(n))
        h = metrics.priority_hash(seed, n)
        assert h.dtype == np.uint64 and [int(x) for x in h] == truth.hash_priorities(seed, n)
        assert np.array_equal(metrics.ReduceDensity(0.1, seed=seed).visiting_order(n), order)
        orders[seed] = order
    assert not np.array_equal(orders[0], orders[1])
    assert not np.array_equal(orders[0], np.arange(n))
    explicit = np.arange(n)[::-1].copy()
    assert np.array_equal(metrics.ReduceDensity(0.1, order=explicit).visiting_order(n), explicit)


def test_argument_errors_are_raised_before_any_device_work():
    """(This machine may have no GPU at all: anything that reached the device would raise
    RaynetHipError, not ValueError.)"""
    from raynet_amd.metrics import ReduceDensity, VoxelMask
    X = truth.uniform_cube(100)
    for bad in (0, -1, -0.5, float("nan")):
        with pytest.raises(ValueError, match="min_dist"):
            ReduceDensity(bad)
    for value in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[1, 17] = value
        with pytest.raises(ValueError, match="non-finite"):
            ReduceDensity(0.1).filter(Y)
    # 21 bits per axis: the message names the axis and the bound
    Y = X.copy()
    Y[2, 3] = 1e-3 * (2 ** 21) * 1.01
    with pytest.raises(ValueError, match=r"axis 2.*below 2097150"):
        ReduceDensity(1e-3).filter(Y)
    for order in (np.arange(99), np.arange(101), np.zeros(100, np.int64),
                  np.r_[np.arange(99), 100], np.r_[np.arange(99), -1],
                  np.arange(100, dtype=np.float64)):
        with pytest.raises(ValueError, match="permutation"):
            ReduceDensity(0.1, order=order).filter(X)
    with pytest.raises(ValueError):
        ReduceDensity(0.1).filter(np.zeros((4, 10)))
    mask = np.ones((2, 2, 2), np.uint8)
    with pytest.raises(ValueError):
        VoxelMask(np.zeros((6,), np.float32), mask)
    with pytest.raises(ValueError):
        VoxelMask(np.array([[0, 0, 0, 1, 0, 1]], np.float32), mask)
    with pytest.raises(ValueError):
        VoxelMask(np.array([[0, 0, 0, 1, 1, 1]], np.float32), mask).filter(np.zeros((2, 5)))


def test_empty_clouds_need_no_device(tmp_path, capsys):
    from raynet_amd.metrics import ReduceDensity, VoxelMask
    empty = np.zeros((3, 0), np.float32)
    for f, name in ((ReduceDensity(0.1, str(tmp_path)), "pc_after_density_reduction.ply"),
                    (VoxelMask(np.array([[0, 0, 0, 1, 1, 1]], np.float32),
                               np.ones((2, 2, 2), np.uint8), str(tmp_path)),
                     "pc_inside_voxel_mask.ply")):
        out = f.filter(empty)
        assert out.shape == (3, 0) and out.dtype == np.float64
        assert "Filter out 0 out of 0 points" in capsys.readouterr().out
        assert open(os.path.join(str(tmp_path), name), "rb").read().endswith(b"end_header\n")


def test_save_colored_ply_round_trips(tmp_path):
    import sys
    from matplotlib import colormaps
    from raynet_amd.pointcloud import Pointcloud
    rng = np.random.default_rng(5)
    X = rng.standard_normal((3, 257))
    intensities = rng.random((257, 1)) * 2.5           # beyond 2: the map saturates
    for cmap in ("jet", "viridis"):
        path = str(tmp_path / ("%s.ply" % cmap))
        Pointcloud(X).save_colored_ply(path, intensities, cmap)
        raw = open(path, "rb").read()
        header, body = raw.split(b"end_header\n", 1)
        assert header.decode().split("\n")[:-1] == [
            "ply", "format binary_%s_endian 1.0" % sys.byteorder, "comment Raynet pointcloud!",
            "element vertex 257", "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue"]
        assert len(body) == 15 * 257
        rec = np.frombuffer(body, dtype=[("xyz", "<f4" if sys.byteorder == "little" else ">f4", 3),
                                         ("rgb", np.uint8, 3)])
        assert np.array_equal(rec["xyz"], X.T.astype(np.float32))
        expected = (colormaps[cmap](intensities.ravel() / 2)[:, :3] * 255).astype(np.uint8)
        assert np.array_equal(rec["rgb"], expected)
    with pytest.raises(ValueError):
        Pointcloud(X).save_colored_ply(str(tmp_path / "bad.ply"), intensities[:5])
