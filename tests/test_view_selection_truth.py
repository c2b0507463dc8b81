"""tests/view_selection_truth.py, the NumPy restatement of rn_view_overlap / rn_view_gain (DESIGN.md
section 30), held to cases worked out by hand: the two exact cases of the band, a ring of cameras
over a plane, an occluder, a back-facing normal, points that are not numbers, a redundancy of two,
and three deliberate mistakes that these cases tell from the definition.  No GPU."""
import numpy as np
import pytest

import view_selection_truth as vt
from appearance_truth import PlaneCamera, pack_cameras

D = np.float64
F = np.float32
SHAPE = (24, 32)
ORIGIN = np.zeros((1, 3), D)


def _pair(c0, c1):
    return pack_cameras([PlaneCamera(*c0, 8.0, 15.5, 11.5), PlaneCamera(*c1, 8.0, 15.5, 11.5)])


def _shared(rows, cos_lo, cos_hi, mutant=None):
    mask, pairs = vt.view_overlap(ORIGIN, None, rows, SHAPE, None, 0.0, 0.0, 0.0, cos_lo, cos_hi,
                                  mutant)
    assert mask.dtype == np.uint64 and pairs.dtype == np.int64
    assert mask.tolist() == [3] and pairs[0, 0] == pairs[1, 1] == 1 and pairs[1, 0] == 0
    return int(pairs[0, 1])


# ------------------------------------------------------------------------------ the band
def test_a_cosine_of_exactly_one_half_is_inside_a_band_that_ends_there():
    """Centres (1, 0, 1) and (0, 1, 1), the point at the origin: dot = 1, q = 4."""
    rows = _pair((1.0, 0.0, 1.0), (0.0, 1.0, 1.0))
    assert _shared(rows, 0.5, 1.0) == 1
    assert _shared(rows, float(np.nextafter(0.5, 1.0)), 1.0) == 0
    assert _shared(rows, 0.0, 0.5) == 1
    assert _shared(rows, 0.0, float(np.nextafter(0.5, 0.0))) == 0
    assert _shared(rows, 0.5, 0.5) == 1


def test_four_fifths_is_decided_on_the_squares_as_computed():
    """Centres (0, 0, 4) and (3, 0, 4): the cosine is 4/5 in exact arithmetic, but 0.8 * 0.8 * 400
    is 256.00000000000006 > 256 -- the pair does NOT count at cos_lo = 0.8."""
    rows = _pair((0.0, 0.0, 4.0), (3.0, 0.0, 4.0))
    assert D(0.8) * D(0.8) * D(400.0) > D(256.0)
    assert _shared(rows, 0.8, 1.0) == 0
    assert _shared(rows, float(np.nextafter(0.8, 0.0)), 1.0) == 1
    assert _shared(rows, 0.0, 0.8) == 1                 # ... and so it is inside a band that ends there


# ------------------------------------------------------------------------------ the ring
@pytest.fixture(scope="module")
def ring():
    cams, rows, points, shape = vt.ring_scene()
    cos_lo, cos_hi = vt.cosines(2.0, 45.0)
    mask, pairs = vt.view_overlap(points, None, rows, shape, None, 0.0, 0.0, 0.0, cos_lo, cos_hi)
    return dict(cams=cams, rows=rows, points=points, shape=shape, mask=mask, pairs=pairs,
                band=(cos_lo, cos_hi))


def test_on_a_ring_the_best_neighbours_are_the_ring_neighbours(ring):
    pairs = vt.symmetric(ring["pairs"])
    assert (np.diag(pairs) > 0).all() and np.array_equal(pairs, pairs.T)
    assert not np.tril(ring["pairs"], -1).any()
    for i in range(8):
        assert sorted(vt.neighbors(pairs, i, 2)) == sorted([(i - 1) % 8, (i + 1) % 8]), i
        assert len(vt.neighbors(pairs, i, 7)) == 7 and i not in vt.neighbors(pairs, i, 7)
        assert (pairs[i] <= pairs[i, i]).all()          # a pair shares no more than either sees


def test_on_a_ring_the_cover_starts_with_two_opposite_cameras(ring):
    order, gains, short = vt.cover(ring["mask"], 8, 8, 1)
    assert len(order) >= 2 and (order[1] - order[0]) % 8 == 4
    seen = np.diag(ring["pairs"])
    assert order[0] == int(np.argmax(seen))             # ties go to the lower index
    assert gains == sorted(gains, reverse=True) and all(g > 0 for g in gains)
    assert gains[0] == int(seen.max())
    seen_by_any = int((ring["mask"] != 0).sum())
    assert sum(gains) == seen_by_any and short == len(ring["points"]) - seen_by_any
    assert len(set(order)) == len(order)
    # stopping at k
    assert vt.cover(ring["mask"], 8, 2, 1)[0] == order[:2]
    assert vt.cover(ring["mask"], 8, 0, 1) == ([], [], len(ring["points"]))
    # candidates
    order35, _, _ = vt.cover(ring["mask"], 8, 8, 1, candidates=[5, 3])
    assert sorted(order35) == [3, 5] or order35 in ([3], [5])


def test_ordering_rules_of_neighbors():
    pairs = vt.symmetric(np.array([[9, 4, 0, 4, 7], [0, 9, 0, 0, 0], [0, 0, 9, 0, 0],
                                   [0, 0, 0, 9, 0], [0, 0, 0, 0, 9]]))
    assert vt.neighbors(pairs, 0, 4) == [4, 1, 3, 2]    # the tie to the lower j, the 0 last
    assert vt.neighbors(pairs, 2, 4) == [0, 1, 3, 4]    # all 0: index order
    assert vt.neighbors(pairs, 0, 2) == [4, 1] and vt.neighbors(pairs, 0, 0) == []


# ------------------------------------------------------------------------------ seeing
def test_a_point_behind_an_occluder_is_not_seen_by_that_view():
    cams = [PlaneCamera(0.0, 0.0, 4.0, 16.0, 8.0, 8.0), PlaneCamera(0.5, 0.0, 4.0, 16.0, 8.0, 8.0)]
    rows = pack_cameras(cams)
    depths = np.full((2,) + SHAPE, 10.0, F)
    depths[0, 8, 8] = 3.0                               # view 0 records something nearer at (8, 8)
    mask, pairs = vt.view_overlap(ORIGIN, None, rows, SHAPE, depths, 0.5, 0.0, 0.0, 0.0, 1.0)
    assert mask.tolist() == [2] and pairs.tolist() == [[0, 0], [0, 1]]
    mask, pairs = vt.view_overlap(ORIGIN, None, rows, SHAPE, depths, 1.0, 0.0, 0.0, 0.0, 1.0)
    assert mask.tolist() == [3] and pairs.tolist() == [[1, 1], [0, 1]]     # dd = 16 <= (3 + 1)^2
    mask, _ = vt.view_overlap(ORIGIN, None, rows, SHAPE, None, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert mask.tolist() == [3]
    for none in (0.0, -1.0, np.nan):
        depths[1] = none
        assert vt.visible(ORIGIN, None, rows, SHAPE, depths, 100.0, 0.0, 0.0).tolist() == [1]


def test_a_back_facing_normal_is_seen_by_nobody_and_a_zero_normal_by_all():
    rows = _pair((1.0, 0.0, 1.0), (0.0, 1.0, 1.0))
    see = lambda n, min_cos=0.0: vt.visible(ORIGIN, np.array([n], D), rows, SHAPE, None, 0.0,  # noqa: E731
                                            min_cos, 0.0).tolist()
    assert see((0, 0, 1)) == [3] and see((0, 0, -1)) == [0] and see((0, 0, 0)) == [3]
    assert see((1, 0, 0)) == [1]                        # perpendicular to view 1's ray: strict
    # cos = 1 / sqrt(2) for both: cos^2 = 1/2 exactly, and the test is strict
    assert see((0, 0, 3), np.sqrt(0.5)) in ([0], [3])
    assert see((0, 0, 3), 0.7) == [3] and see((0, 0, 3), 0.71) == [0]


def test_points_that_are_not_numbers_set_no_bit():
    cams, rows, points, shape = vt.ring_scene(side=5)
    depths = vt.analytic_depths(cams, *shape)
    points = points.copy()
    points[3, 0], points[7, 1], points[11, 2], points[12] = np.nan, np.inf, -np.inf, np.nan
    for dm in (None, depths):
        for nr in (None, np.tile([0.0, 0.0, 1.0], (len(points), 1))):
            mask, pairs = vt.view_overlap(points, nr, rows, shape, dm, 0.1, 0.0, 0.0, 0.0, 1.0)
            assert not mask[[3, 7, 11, 12]].any() and mask.any()
            assert pairs.trace() == int(vt.popcount(mask).sum())


# ------------------------------------------------------------------------------ gains
MASKS = np.array([0b0001, 0b0011, 0b0111, 0b1000, 0b0000, 0b1111, 0b0110], np.uint64)


def test_gain_counts_the_short_points_each_candidate_sees():
    assert vt.gain(MASKS, 4, 0, 1).tolist() == [4, 4, 3, 2, 7]
    assert vt.gain(MASKS, 4, 0b0001, 1).tolist() == [0, 1, 1, 1, 3]
    assert vt.gain(MASKS, 4, 0b1111, 1).tolist() == [0, 0, 0, 0, 1]
    # bits of chosen at V and above play no part; bits of the masks there neither
    assert vt.gain(MASKS, 3, 0b1000, 1).tolist() == [4, 4, 3, 7]
    assert vt.gain(MASKS, 3, 0b1001, 1).tolist() == [0, 1, 1, 3]


def test_redundancy_two_keeps_a_point_short_until_two_chosen_views_see_it():
    assert vt.gain(MASKS, 4, 0b0001, 2).tolist() == [0, 4, 3, 2, 7]
    assert vt.gain(MASKS, 4, 0b0011, 2).tolist() == [0, 0, 1, 1, 4]
    order, gains, short = vt.cover(MASKS, 4, 4, 2)
    assert order == [0, 1, 2, 3] and gains == [4, 4, 1, 1]
    # 0001 and 1000 have one view each, 0000 none: short for ever at redundancy 2
    assert short == 3
    assert vt.gain(MASKS, 4, 0b1111, 64).tolist() == [0, 0, 0, 0, 7]


def test_the_popcount_and_the_top_bit():
    top = np.array([1 << 63, (1 << 64) - 1, 0, (1 << 63) | 1], np.uint64)
    assert vt.popcount(top).tolist() == [1, 64, 0, 2]
    assert vt.bit(top, 63).tolist() == [True, True, False, True]
    g = vt.gain(top, 64, 0, 1)
    assert g[63] == 3 and g[0] == 2 and g[64] == 4
    assert vt.gain(top, 64, 1 << 63, 1)[64] == 1 and vt.gain(top, 64, -1, 1)[:64].sum() == 0
    assert vt.low_bits(64) == np.uint64(0xFFFFFFFFFFFFFFFF) and vt.low_bits(3) == 7


# ------------------------------------------------------------------------------ the mutants
def test_three_mistakes_are_told_from_the_definition(ring):
    # the band on c instead of c c: the exact case of one half
    rows = _pair((1.0, 0.0, 1.0), (0.0, 1.0, 1.0))
    assert _shared(rows, 0.5, 1.0) == 1 and _shared(rows, 0.5, 1.0, "band_on_c") == 0
    # a pair counted when one of the two sees the point: the occluder's case
    cams = [PlaneCamera(0.0, 0.0, 4.0, 16.0, 8.0, 8.0), PlaneCamera(0.5, 0.0, 4.0, 16.0, 8.0, 8.0)]
    depths = np.full((2,) + SHAPE, 10.0, F)
    depths[0, 8, 8] = 3.0
    args = (ORIGIN, None, pack_cameras(cams), SHAPE, depths, 0.5, 0.0, 0.0, 0.0, 1.0)
    assert vt.view_overlap(*args)[1][0, 1] == 0 and vt.view_overlap(*args, "one_sees")[1][0, 1] == 1
    # ... and the ring tells both as well
    for mutant in ("band_on_c", "one_sees"):
        wrong = vt.pair_counts(ring["points"], ring["mask"], ring["rows"], *ring["band"], mutant)
        assert not np.array_equal(wrong, ring["pairs"]), mutant
    # chosen ignored in the short test
    assert vt.gain(MASKS, 4, 0b0001, 1).tolist() != vt.gain(MASKS, 4, 0b0001, 1, "chosen_ignored").tolist()
    assert vt.cover(ring["mask"], 8, 8, 1)[0] != vt.cover(ring["mask"], 8, 8, 1, mutant="chosen_ignored")[0]
