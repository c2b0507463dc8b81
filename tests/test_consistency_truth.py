"""tests/consistency_truth.py, the NumPy restatement of rn_points_consistency (DESIGN.md section
29), without a GPU: hand-made cases on the perturbed plane scene -- three cameras over z = 0, height
3, focal 20, 24 x 32, a floater (depth x 0.7) and a dent (depth x 1.2) planted in view 0 -- and two
mutants of the definition that these cases tell from it."""
import numpy as np
import pytest

import consistency_truth as ct
from appearance_truth import PlaneCamera, pack_cameras

F = np.float32
D = np.float64
TOLERANCES = [(0.08, 0.0), (0.0, 0.025)]


@pytest.fixture(scope="module")
def scene():
    cams, rows, depths, kind = ct.perturbed_plane_scene()
    points = ct.back_project(cams[0], depths[0])
    return dict(cams=cams, rows=rows, depths=depths, kind=kind.reshape(-1), points=points,
                own=depths[0].reshape(-1))


def _check(scene, tol_abs, tol_rel, exclude=0, **mutant):
    return ct.check_points(scene["points"], scene["rows"], scene["depths"], exclude, tol_abs,
                           tol_rel, 0.0, **mutant)


@pytest.mark.parametrize("tol_abs,tol_rel", TOLERANCES)
def test_untouched_floater_and_dent(scene, tol_abs, tol_rel):
    seen, agree, violate, residual = _check(scene, tol_abs, tol_rel)
    kind = scene["kind"]
    assert seen.dtype == agree.dtype == violate.dtype == np.uint32 and residual.dtype == F
    assert not ((seen | agree | violate) & 1).any()                 # view 0 is excluded
    assert not (agree & ~seen).any() and not (violate & ~seen).any() and not (agree & violate).any()
    untouched, floater, dent = kind == 0, kind == 1, kind == 2
    assert floater.sum() == 16 and dent.sum() == 12
    # every untouched pixel: whoever measures agrees, nobody is violated
    assert np.array_equal(agree[untouched], seen[untouched]) and not violate[untouched].any()
    # every floater pixel: both other views see past it
    assert (ct.popcount(seen[floater]) == 2).all()
    assert np.array_equal(violate[floater], seen[floater]) and not agree[floater].any()
    # every dent pixel: both other views measure, neither agrees, neither is violated (occluded)
    assert (ct.popcount(seen[dent]) == 2).all()
    assert not agree[dent].any() and not violate[dent].any()
    # 78 untouched pixels are seen by no other view: one agreeing view asked, they go
    assert int((seen[untouched] == 0).sum()) == 78
    kept = ct.keep(scene["own"], agree, violate, min_views=1)
    assert int(kept.sum()) == 768 - 16 - 12 - 78
    assert not kept[floater].any() and not kept[dent].any() and not kept[seen == 0].any()
    assert kept[untouched & (seen != 0)].all()
    # the residual of every untouched pixel lies within the tolerance
    # (each agreeing view's |s| is at most its own t = tol_abs + tol_rel z, and so is their mean)
    t = tol_abs + tol_rel * scene["depths"][1:].astype(D).max()
    print("tol_abs %g tol_rel %g: |residual| of the untouched pixels up to %.6f"
          % (tol_abs, tol_rel, np.abs(residual[untouched]).max()))
    assert (np.abs(residual[untouched]) <= t).all()
    assert (residual[ct.popcount(agree) == 0] == 0).all()


def test_a_tolerance_below_one_pixels_depth_step_violates_a_slanted_plane(scene):
    """The documented caveat: the depth is read at the nearest pixel, and half a pixel of this
    plane, slanted against the rays, is up to about 0.05 of depth.  At tol_abs = 0.04 untouched
    pixels -- 15 of them -- are violated by views that see the very same plane."""
    seen, agree, violate, _ = _check(scene, 0.04, 0.0)
    untouched = scene["kind"] == 0
    assert int((violate[untouched] != 0).sum()) == 15
    assert not np.array_equal(agree[untouched], seen[untouched])
    # ... and at a tolerance far below it, the residual is 0 wherever no view agrees
    seen, agree, violate, residual = _check(scene, 1e-5, 0.0)
    none = ct.popcount(agree) == 0
    assert none.sum() > 500 and (residual[none] == 0).all() and not np.signbit(residual[none]).any()
    assert (np.abs(residual[~none]) <= 1e-5).all()


def test_without_exclusion_a_view_agrees_with_itself(scene):
    """exclude = -1: view 0 is asked about its own points.  Wherever it measures it agrees, floater
    and dent included, at a tolerance of 1e-6 (the camera rows carry the centre the camera object
    holds, which is float32: 0.35 is 1e-8 off there); it measures at every interior pixel (the
    projection of a pixel on the image's edge lands within an ulp of the edge, on either side).
    The other views' bits are what they were."""
    seen, agree, violate, residual = _check(scene, 1e-6, 0.0, exclude=-1)
    assert np.array_equal(agree & 1, seen & 1) and not (violate & 1).any()
    interior = np.zeros((24, 32), bool)
    interior[1:-1, 1:-1] = True
    assert ((seen & 1) == 1)[interior.reshape(-1)].all()
    with_, without = _check(scene, 0.08, 0.0, exclude=-1), _check(scene, 0.08, 0.0, exclude=0)
    for a, b in zip(with_[:3], without[:3]):
        assert np.array_equal(a & ~np.uint32(1), b)
    # s is exactly 0 where the arithmetic is exact: a camera at (0, 0, 4) that sends (x, y, 0) to
    # (4 x + 8, 4 y + 8), the points under pixels (8, 8) and (20, 8) at their own depths 4 and 5
    cam = PlaneCamera(0.0, 0.0, 4.0, 16.0, 8.0, 8.0)
    depths = np.full((1, 24, 32), 7.0, F)
    depths[0, 8, 8], depths[0, 8, 20] = 4.0, 5.0
    points = np.array([[0.0, 3.0], [0.0, 0.0], [0.0, 0.0]], D)
    seen, agree, violate, residual = ct.check_points(points, pack_cameras([cam]), depths, -1, 0.0,
                                                     0.0, 0.0)
    assert (seen == 1).all() and (agree == 1).all() and (violate == 0).all()
    assert (residual == 0).all()
    # ... and with the view excluded nothing is set
    for out in ct.check_points(points, pack_cameras([cam]), depths, 0, 0.0, 0.0, 0.0):
        assert (out == 0).all()


def test_the_bounds_of_the_band_belong_to_it():
    """zm = 2, dd = 1 gives s = (4 - 1) / 4 = 0.75 exactly; zm = 2, dd = 9 gives s = -1.25."""
    cam = PlaneCamera(0.0, 0.0, 4.0, 16.0, 8.0, 8.0)
    rows = pack_cameras([cam])
    depths = np.full((1, 24, 32), 2.0, F)
    for point, s in (((0.0, 0.0, 3.0), 0.75), ((0.0, 0.0, 1.0), -1.25)):
        p = np.array(point, D).reshape(3, 1)
        at, below = abs(s), np.nextafter(abs(s), 0.0)
        seen, agree, violate, residual = ct.check_points(p, rows, depths, -1, at, 0.0, 0.0)
        assert (seen[0], agree[0], violate[0], residual[0]) == (1, 1, 0, F(s))
        seen, agree, violate, residual = ct.check_points(p, rows, depths, -1, below, 0.0, 0.0)
        assert (seen[0], agree[0], violate[0], residual[0]) == (1, 0, 1 if s > 0 else 0, 0)
        # the same bound as a relative tolerance: t = tol_rel * 2
        seen, agree, violate, _ = ct.check_points(p, rows, depths, -1, 0.0, at / 2, 0.0)
        assert (seen[0], agree[0], violate[0]) == (1, 1, 0)


def test_what_holds_no_measurement_is_never_kept():
    depth = np.array([1.0, 0.0, -1.0, np.nan, np.inf, 2.0], F)
    agree = np.array([3, 3, 3, 3, 3, 1], np.uint32)
    violate = np.array([0, 0, 0, 0, 0, 0x80000000], np.uint32)
    assert ct.keep(depth, agree, violate).tolist() == [True, False, False, False, False, False]
    assert ct.keep(depth, agree, violate, 1, 1).tolist() == [True, False, False, False, False, True]
    assert ct.popcount(np.array([0, 1, 0x80000001, 0xFFFFFFFF], np.uint32)).tolist() == [0, 1, 2, 32]


# ------------------------------------------------------------------------------ the mutants
def test_a_mutant_that_swaps_violated_and_occluded_fails(scene):
    _, agree, violate, _ = _check(scene, 0.08, 0.0, swap_signs=True)
    floater, dent = scene["kind"] == 1, scene["kind"] == 2
    # it calls the floater occluded and the dent violated: the floater's assertion fails
    assert not violate[floater].any() and (ct.popcount(violate[dent]) == 2).all()
    _, _, right, _ = _check(scene, 0.08, 0.0)
    assert not np.array_equal(violate, right)


def test_a_mutant_that_does_not_skip_the_excluded_view_fails(scene):
    seen, agree, _, _ = _check(scene, 0.08, 0.0, skip_exclude=False)
    assert (seen & 1).any() and (agree & 1).any()          # view 0 answered
    # ... so the floater and the dent each have an agreeing view, and are kept
    kept = ct.keep(scene["own"], agree, np.zeros_like(agree), min_views=1)
    assert kept[scene["kind"] == 2].all()
