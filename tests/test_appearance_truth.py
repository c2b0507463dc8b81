"""tests/appearance_truth.py held to properties nobody has to trust (no GPU): colours of a plane
whose colour field bilinear interpolation reproduces exactly, an occluder that removes one view
from exactly the points behind it, and normals of closed surfaces."""
import numpy as np
import pytest

import appearance_truth as at
import isosurface_truth as it

F = np.float32
TOL = 0.1       # scene units: a pixel's footprint on the plane is 3 / 20 = 0.15, and the depth
                # changes by less than 0.7 of the way across the ground, so half a pixel's
                # diagonal (0.106) moves it by less than 0.08


@pytest.fixture(scope="module")
def plane():
    cams, images, depths = at.plane_scene()
    rng = np.random.default_rng(11)
    pts = np.zeros((500, 3), F)
    pts[:, 0] = rng.uniform(-3.0, 3.0, 500)
    pts[:, 1] = rng.uniform(-2.4, 2.4, 500)
    return cams, at.pack_cameras(cams), images, depths, pts


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("with_normals", [False, True])
def test_affine_plane_gets_its_own_colours(plane, mode, with_normals):
    cams, packed, images, depths, pts = plane
    assert images.shape == (3, 24, 32, 3) and images.min() >= 0 and images.max() <= 1
    normals = np.tile(np.array([0, 0, 2], F), (len(pts), 1)) if with_normals else None
    colors, weight, views = at.project_colors(pts, normals, packed, images, depths, TOL, 0.0, 0.0,
                                              mode)
    assert colors.dtype == F and weight.dtype == F and views.dtype == np.uint32
    seen = views != 0
    want = at.affine_field(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    err = np.abs(colors[seen].astype(np.float64) - want[seen]).max()
    print("mode %d, normals %s: %d of %d seen, max error %.3g" % (mode, with_normals, seen.sum(),
                                                                  len(pts), err))
    assert err <= 1e-6
    assert sorted(set(views.tolist())) == list(range(8)), "all eight view masks occur"
    assert (colors[~seen] == 0).all() and (weight[~seen] == 0).all() and (~seen).any()
    # the mask is what the geometry says: a view sees the points that project into its image
    for v, cam in enumerate(cams):
        X = cam.focal * (pts[:, 0].astype(np.float64) - cam.cx) / cam.height + cam.u0
        Y = cam.focal * (pts[:, 1].astype(np.float64) - cam.cy) / cam.height + cam.v0
        inside = (X >= 0) & (X <= 31) & (Y >= 0) & (Y <= 23)
        clear = (np.abs(X - 15.5) < 15.49) & (np.abs(Y - 11.5) < 11.49) | ~inside
        assert np.array_equal(((views >> v) & 1).astype(bool)[clear], inside[clear])
    if not with_normals:
        assert np.array_equal(weight, np.array([bin(m).count("1") for m in views], F))
    else:
        assert (weight[seen] > 0).all() and (weight <= 3).all()


def test_an_occluder_removes_one_view_from_exactly_the_points_behind_it(plane):
    cams, packed, images, depths, pts = plane
    _, _, before = at.project_colors(pts, None, packed, images, depths, TOL, 0.0, 0.0, 0)
    blocked = depths.copy()
    blocked[0, :, :16] *= F(0.5)
    _, _, after = at.project_colors(pts, None, packed, images, blocked, TOL, 0.0, 0.0, 0)
    cam = cams[0]
    X = cam.focal * (pts[:, 0].astype(np.float64) - cam.cx) / cam.height + cam.u0
    behind = ((before & 1) == 1) & (np.rint(X) < 16)
    print("%d points lose view 0" % behind.sum())
    assert behind.sum() > 50 and (((before & 1) == 1) & ~behind).sum() > 50
    assert np.array_equal(after & 1, np.where(behind, 0, before & 1))
    assert np.array_equal(after & ~np.uint32(1), before & ~np.uint32(1))


def test_one_sided_occlusion_and_special_depths(plane):
    cams, packed, images, depths, pts = plane
    raised = pts.copy()
    raised[:, 2] = 0.5                                  # in front of the recorded surface: seen
    _, _, views = at.project_colors(raised, None, packed, images, depths, 0.0, 0.0, 0.0, 0)
    _, _, free = at.project_colors(raised, None, packed, images, None, 0.0, 0.0, 0.0, 0)
    assert np.array_equal(views, free) and (views != 0).any()
    sunk = pts.copy()
    sunk[:, 2] = -0.5                                   # behind it: hidden
    _, _, views = at.project_colors(sunk, None, packed, images, depths, TOL, 0.0, 0.0, 0)
    assert (views == 0).all()
    for value, hides in ((np.inf, False), (0.0, True), (-1.0, True), (np.nan, True)):
        d = np.full_like(depths, value)
        _, _, views = at.project_colors(sunk, None, packed, images, d, TOL, 0.0, 0.0, 0)
        _, _, free = at.project_colors(sunk, None, packed, images, None, TOL, 0.0, 0.0, 0)
        assert (views == 0).all() if hides else np.array_equal(views, free), value


@pytest.mark.parametrize("mode", [0, 1])
def test_planted_points_meet_the_conditions_worked_out_by_hand(mode):
    scene = at.planted_scene()
    got = at.project_colors(scene["points"], scene["normals"], scene["cameras"], scene["images"],
                            scene["depths"], 0.0, 0.0, 0.0, mode)
    at.check_planted(got, scene, mode)
    # half to even: with the lookup rounding half away from zero, X = 0.5 and 2.5 would be hidden
    assert scene["depths"][0, 8, 1] == 0 and scene["depths"][0, 8, 3] == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_no_normals_and_zero_normals_are_the_same_bits(plane, mode):
    """normals=None and an all-zero normal array (of either sign) are one spelling: no facing
    test, every view weighs 1 -- through project_colors's float32 door and observe's float64 one."""
    D = np.float64
    cams, packed, images, depths, pts = plane
    scene = at.planted_scene()
    for points, rows, pictures, maps in (
            (pts, packed, images, depths), (pts, packed, images, None),
            (scene["points"], scene["cameras"], scene["images"], scene["depths"])):
        none = at.project_colors(points, None, rows, pictures, maps, TOL, 0.3, 0.5, mode)
        assert (none[2] != 0).any()
        for entry, cast in ((at.project_colors, F), (at.observe, D)):
            for zero in (0.0, -0.0):
                got = entry(points.astype(cast), np.full(points.shape, zero, cast), rows,
                            pictures, maps, TOL, 0.3, 0.5, mode)
                assert np.array_equal(got[0].view(np.int32), none[0].view(np.int32))
                assert np.array_equal(got[1].view(np.int32), none[1].view(np.int32))
                assert np.array_equal(got[2], none[2]) and got[2].dtype == np.uint32
        assert np.array_equal(none[1], np.rint(none[1]))       # whole weights: one per view


# ------------------------------------------------------------------------------- the normals
def _ball():
    belief = it.logistic_ball()
    bbox, axes = it.unit_frame(belief.shape)
    return it.extract(belief, 0.5, True, axes, bbox)


def test_normals_of_the_ball_point_outwards_and_sum_to_zero():
    v, f = _ball()
    assert (len(v), len(f)) == (756, 1508)
    val = at.valence(f, len(v))
    assert val.min() >= 4 and val.max() <= 9
    n = at.area_normals(v, f)
    assert n.dtype == F and n.shape == v.shape
    length = np.sqrt((n.astype(np.float64) ** 2).sum(1))
    assert (length > 0).all()
    radial = v.astype(np.float64) - np.array([5.3, 5.1, 4.6])
    cos = (n * radial).sum(1) / length / np.sqrt((radial ** 2).sum(1))
    print("cosine to the radial direction: min %.3f mean %.3f" % (cos.min(), cos.mean()))
    assert cos.min() >= 0.95
    total = np.abs(n.astype(np.float64).sum(0))
    print("sum of the area normals: %s" % total)
    assert (total <= 1e-5).all()


def test_normals_of_the_noise_mesh_have_exact_zeros():
    belief = it.noise()
    bbox, axes = it.unit_frame(belief.shape)
    v, f = it.extract(belief, 0.5, True, axes, bbox)
    n = at.area_normals(v, f)
    zero = (n == 0).all(1)
    print("%d of %d normals are zero" % (zero.sum(), len(n)))
    assert np.isfinite(n).all() and zero.any() and not zero.all()
    assert np.array_equal(n[zero].view(np.int32) & 0x7fffffff, np.zeros((zero.sum(), 3), np.int32))


def test_tetrahedron_normals_point_away_from_the_centroid():
    v, f = at.tetrahedron()
    assert it.signed_volume(v, f) > 0
    n = at.area_normals(v, f)
    centroid = v.astype(np.float64).mean(0)
    assert ((n * (v - centroid)).sum(1) > 0).all()
    # three faces of area 2 sqrt(3) meet at a vertex; their normals add up along the vertex
    assert np.allclose(n, v * 4.0)


def test_unused_vertices_and_bad_indices_are_skipped():
    v, f = at.tetrahedron()
    v5 = np.concatenate([v, [[9, 9, 9]]]).astype(F)
    n = at.area_normals(v5, f)
    assert np.array_equal(n[:4], at.area_normals(v, f)) and (n[4] == 0).all()
    offsets, corners = at.corner_table(f, 5)
    assert offsets.tolist() == [0, 3, 6, 9, 12, 12] and corners.tolist()[:3] == [0, 3, 6]
    broken = corners.copy()
    broken[1] = 99                  # a corner beyond 3 nf: vertex 0 loses that face only
    got = at.area_normals(v5, f, offsets, broken)
    assert np.array_equal(got[1:], n[1:]) and not np.array_equal(got[0], n[0])
    bad_faces = f.copy()
    bad_faces[3, 1] = 7             # a face with a vertex beyond nv: skipped where it is named
    got = at.area_normals(v5, bad_faces, offsets, corners)
    assert np.array_equal(got[0], n[0]) and np.isfinite(got).all()
