"""tests/scatter_truth.py held to hand-made closed forms (CPU), and the route floors of the
fixtures of tests/test_scatter_paths_gpu.py, which depend on host data alone."""
import numpy as np
import pytest

import scatter_truth as T


def _rays(*rays, M=4):
    """lists [n][M][3], counts [n] from per-ray lists of voxels."""
    lists = np.zeros((len(rays), M, 3), np.int32)
    counts = np.zeros(len(rays), np.int32)
    for r, vox in enumerate(rays):
        counts[r] = len(vox)
        for i, v in enumerate(vox[:M]):
            lists[r, i] = v
    return lists, counts


def test_fixed_rounds_ties_to_even():
    u = 2.0 ** -32
    m = np.array([0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, 0.75 * u, 1.0, -3.25],
                 np.float32)
    assert np.array_equal(m.astype(np.float64), [0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u,
                                                 -2.5 * u, 0.75 * u, 1.0, -3.25])      # all exact in fp32
    got = T.fixed(m)
    assert got.dtype == np.int64
    assert got.tolist() == [0, 2, 2, 0, -2, -2, 1, 1 << 32, -13 * (1 << 30)]
    with pytest.raises(AssertionError):
        T.fixed(np.array([np.inf], np.float32))


def test_two_rays_through_one_voxel_and_a_ray_that_sends_nothing():
    grid = (3, 4, 5)
    lists, counts = _rays([(1, 2, 3), (1, 2, 4)], [(0, 2, 3), (1, 2, 3), (2, 2, 3)], [(2, 3, 4)])
    msgs = np.array([[0.5, -0.25, 9, 9], [2.0, 1.5 * 2.0 ** -32, -1.0, 9], [7.0, 9, 9, 9]], np.float32)
    want = np.zeros(grid, np.int64)
    want[1, 2, 3] = (1 << 31) + 2               # 0.5 and the tie 1.5 -> 2
    want[1, 2, 4] = -(1 << 30)
    want[0, 2, 3] = 2 << 32
    want[2, 2, 3] = -(1 << 32)
    # ray 2 has one voxel: its message (7.0 at (2, 3, 4)) is not summed; nor is anything past a count
    got = T.partial_fixed(msgs, lists, counts, grid)
    assert np.array_equal(got, want)
    assert np.array_equal(T.partial_fixed(msgs, ((lists[..., 0] << 20) | (lists[..., 1] << 10) | lists[..., 2]),
                                          counts, grid), want)                 # packed lists
    total, n_v, a_v = T.partial_f64(msgs, lists, counts, grid)
    assert n_v.sum() == 5 and n_v[1, 2, 3] == 2 and n_v[2, 3, 4] == 0
    assert total[1, 2, 3] == 0.5 + 1.5 * 2.0 ** -32 and a_v[1, 2, 4] == 0.25 and total[1, 2, 4] == -0.25
    assert a_v[2, 2, 3] == 1.0 and total[2, 2, 3] == -1.0 and total[2, 3, 4] == 0 and a_v[2, 3, 4] == 0
    # a count above M sends M messages
    counts[1] = 9
    assert T.sending(counts, 4).tolist() == [2, 4, 0]
    assert T.sending(counts, 2).tolist() == [2, 2, 0]


def test_brick_index_in_a_partial_brick():
    grid = (5, 6, 7)                            # 2 x 2 x 2 bricks, the last of each axis partial
    assert int(T.brick_index(4, 5, 6, grid)) == ((1 * 2 + 1) * 2 + 1) * 64 + (0 << 4 | 1 << 2 | 2) == 454
    assert int(T.brick_index(0, 0, 0, grid)) == 0 and int(T.brick_index(3, 3, 3, grid)) == 63
    assert int(T.brick_index(0, 0, 4, grid)) == 64 and int(T.brick_index(0, 4, 0, grid)) == 128
    X, Y, Z = np.meshgrid(np.arange(5), np.arange(6), np.arange(7), indexing="ij")
    at = T.brick_index(X, Y, Z, grid)
    assert len(np.unique(at)) == 5 * 6 * 7 and at.min() == 0 and at.max() < 2 * 2 * 2 * 64
    acc = np.zeros(512, np.int64)
    acc[454] = 11
    acc[455] = 5                                # (4, 5, 7): no voxel of the grid
    got, stray = T.from_bricked(acc, grid)
    assert got[4, 5, 6] == 11 and got.sum() == 11 and stray == 1


@pytest.mark.parametrize("level,far,volume", [
    (0, (15, 15, 15), 4096),                    # 16 x 16 x 16 = CAP: fits
    (0, (16, 240, 0), 4097),                    # 17 x 241 x 1 = CAP + 1: overflows
    (1, (15, 15, 23), 6144),                    # 16 x 16 x 24 = CAP: fits
    (1, (13, 438, 0), 6146),                    # 14 x 439 x 1: the smallest box above CAP with
])                                              # sides below 1024 (6145 = 5 x 1229)
def test_census_at_the_capacity_of_the_box(level, far, volume):
    RAYS, STEPS, CAP = T.LEVELS[level]
    near = (0, 0, 0)
    step_back = tuple(f - 1 if f else 0 for f in far)
    lists, counts = _rays([near, near], [far, step_back], M=STEPS)
    # rows 0 and 1 of one tile, both voxels of each ray in the first quarter
    c = T.census(lists, counts, STEPS, level)
    assert c["chunks"] == 1 and c["volume"][0, 0] == volume
    if volume <= CAP:
        assert (c["overflowed"], c["in_box"], c["fit"], c["nofit"]) == (0, 1, 0, 0)
    else:
        assert (c["overflowed"], c["in_box"], c["fit"], c["nofit"]) == (1, 0, 0, 1)
        assert c["pieces"] == [(0, 0, 0, volume)]


def test_census_quarters_and_tiles():
    """Level 0: a second tile whose chunk overflows although each of its quarters fits; rays that
    send nothing open no chunk."""
    M = 64
    lists = np.zeros((130, M, 3), np.int32)
    counts = np.zeros(130, np.int32)
    counts[3] = 1                                                   # tile 0: nothing is sent
    lists[128, :40] = [(0, 0, s) for s in range(40)]                # tile 1: 2 chunks
    lists[129, :20] = [(40, 40, s) for s in range(20)]
    counts[128], counts[129] = 40, 20
    c = T.census(lists, counts, M, 0)
    assert c["chunks"] == 2 and c["overflowed"] == 1
    assert c["volume"].tolist() == [[-1, -1], [41 * 41 * 32, 8]]
    # quarters of chunk 0: steps 0-7, 8-15 (both rays: 41 x 41 x 8), 16-23 (ray 129 has 4 left:
    # the box spans z 16..23), 24-31 (ray 128 alone: 8 voxels)
    assert c["pieces"] == [(1, 0, 0, 13448), (1, 0, 1, 13448), (1, 0, 2, 13448), (1, 0, 3, 8)]
    assert (c["fit"], c["nofit"]) == (1, 3)
    c1 = T.census(lists, counts, M, 1)                              # one tile of 256 rows, 16 steps
    assert c1["chunks"] == 3 and c1["overflowed"] == 2 and c1["volume"].tolist() == [[26896, 26896, 8, -1]]


def test_slab_table_and_the_merge_of_its_boxes():
    M = 48
    lists = np.zeros((130, M, 3), np.int32)
    counts = np.zeros(130, np.int32)
    lists[0, :20] = [(5, 5, 10 + s) for s in range(20)]             # block 0: slabs 0 and 1
    lists[1, 0] = (9, 2, 3)                                         # one voxel: in the box, sends nothing
    lists[64, :10] = [(30 - s, 7, 7) for s in range(10)]            # block 1: slab 0, x falling
    counts[0], counts[1], counts[64] = 20, 1, 10
    tab = T.slab_table(lists, counts, M)
    pk = lambda x, y, z: (x << 20) | (y << 10) | z
    assert tab.shape == (3, 3, 2) and tab.dtype == np.int32
    assert tab[0, 0].tolist() == [pk(5, 2, 3), pk(9, 5, 25)]
    assert tab[0, 1].tolist() == [pk(5, 5, 26), pk(5, 5, 29)]
    assert tab[1, 0].tolist() == [pk(21, 7, 7), pk(30, 7, 7)]
    for b, s in ((0, 2), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)):
        assert tuple(tab[b, s]) == T.EMPTY_SLAB
    # level 0: tile 0 = blocks 0 and 1, chunk 0 = slabs 0 and 1 of each.  A stale entry where the
    # traversal wrote nothing (block 1, slab 1: beyond that half's longest sending ray) is not read
    stale = tab.copy()
    stale[1, 1] = [pk(0, 0, 0), pk(1000, 1000, 1000)]
    for t in (tab, stale):
        c = T.census(lists, counts, M, 0, t)
        assert c["chunks"] == 1 and c["volume"][0, 0] == (30 - 5 + 1) * (7 - 2 + 1) * (29 - 3 + 1) == 4212
        assert c["overflowed"] == 1 and c["pieces"] == [(0, 0, 0, 5 * 4 * 23), (0, 0, 1, 4), (0, 0, 2, 10)]
        assert (c["fit"], c["nofit"]) == (3, 0)
    # the exact boxes leave the one-voxel ray out: 26 x 3 x 23 fits
    assert T.census(lists, counts, M, 0)["volume"][0, 0] == 26 * 3 * 23
    assert T.census(lists, counts, M, 0)["overflowed"] == 0
    # an entry with a negative second word is empty even where it is read
    holed = tab.copy()
    holed[1, 0, 1] = -1
    assert T.census(lists, counts, M, 0, holed)["volume"][0, 0] == 5 * 4 * 27
    # level 1: 256 rows x 16 steps, blocks 0..3 (block 3 lies beyond the table: empty)
    c = T.census(lists, counts, M, 1, tab)
    assert c["chunks"] == 2 and c["volume"].tolist() == [[26 * 6 * 23, 4, -1]] and c["overflowed"] == 0


def test_route_floors_of_the_gpu_fixtures():
    """Every scene of tests/test_scatter_paths_gpu.py has the routes it is named after, by the
    host census alone, at both tile shapes."""
    import test_scatter_paths_gpu as G
    for table in (G.PINHOLE, G.PINHOLE_ODD):
        for name, (grid, M, spacing) in table.items():
            for rows in (1024, 1000):
                lists, counts = G.pinhole_lists(grid, M, spacing, rows)
                for level in (0, 1):
                    G.route_floor(name, T.census(lists, counts, M, level))
    for name, (grid, M, focal) in G.RING.items():
        lists, counts, _ = G.ring_lists(grid, M, focal)
        tab = T.slab_table(lists, counts, M)
        for level in (0, 1):
            c = T.census(lists, counts, M, level, tab)
            G.route_floor(name, c)
            assert c["overflowed"] >= T.census(lists, counts, M, level)["overflowed"]
            assert name != "medium" or c["nofit"] == 0
    lists, counts, grid, M, _ = G.field_limit_lists()
    assert -(-int(T.sending(counts, M).max()) // 16) == 64          # a first chunk of 63 exists
