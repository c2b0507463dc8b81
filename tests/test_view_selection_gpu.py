"""View selection on the GPU: rn_view_overlap and rn_view_gain against
tests/view_selection_truth.py -- the masks, the pair matrix and the gains as integers, every entry,
no tolerance -- over the sizes at which a launch can go wrong (one lane, a wavefront and a block
more or less, more tiles than the block cap), 1 to 64 views, with and without normals and depth
maps, wavefronts in which no lane or one lane sees a view, points that are not numbers, the exact
cases of the band, the entries behind and below the outputs, calls over halves of a cloud, the
package's cover and best_frames, and the refusals of both entries."""
import ctypes

import numpy as np
import pytest

import view_selection_truth as vt
from appearance_truth import PlaneCamera, pack_cameras
from mesh_harness import PAD, assert_untouched, cuda

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
VISIBLE_FILL, PAIRS_FILL, GAIN_FILL = -7, 1000, 500
CAP = 1024 * 256                        # the block cap times the block size: raynet_overlap_args.h


def _ctx():
    from raynet_amd.hip_implementations import get_context
    return get_context()


def _overlap(points, normals, rows, shape, depths, tol=0.0, min_cos=0.0, border=0.0, cos_lo=0.0,
             cos_hi=1.0, pairs=None):
    """rn_view_overlap on points [n, 3] with visible PAD entries and pairs PAD rows longer than
    asked for and prefilled -> (visible uint64 [n], what was ADDED to pairs [V, V] int64), after
    checking that the PAD entries and the lower triangle kept their prefill.  pairs: the device
    matrix of an earlier call, to be added to."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = _ctx()
    points = np.ascontiguousarray(points, D).reshape(-1, 3)
    n, V = len(points), len(rows)
    H, W = shape
    d_points = cuda(points.T, D)
    d_normals = None if normals is None else cuda(np.asarray(normals, D).reshape(-1, 3).T, D)
    d_depths = None if depths is None else cuda(depths, F)
    d_rows = cuda(rows, D)
    visible = torch.full((n + PAD,), VISIBLE_FILL, dtype=torch.int64, device="cuda")
    before = None
    if pairs is None:
        pairs = torch.full((V + PAD, V), PAIRS_FILL, dtype=torch.int64, device="cuda")
    else:
        before = pairs.cpu().numpy()[:V].copy()
    ctx._check(ctx.lib.rn_view_overlap(
        ctx._h, n, _ptr(d_points), _ptr(d_normals), V, _ptr(d_rows), H, W, _ptr(d_depths),
        float(tol), float(min_cos), float(border), float(cos_lo), float(cos_hi), _ptr(visible),
        _ptr(pairs), _stream()))
    assert_untouched(visible, n, np.int64(VISIBLE_FILL), "visible")
    assert_untouched(pairs, V, np.int64(PAIRS_FILL), "pairs")
    got = pairs.cpu().numpy()[:V]
    added = got - (PAIRS_FILL if before is None else before)
    assert not np.tril(added, -1).any(), "the lower triangle was written"
    return visible.cpu().numpy()[:n].view(np.uint64), added, pairs


def _held_to_the_truth(points, normals, rows, shape, depths, tol=0.0, min_cos=0.0, border=0.0,
                       cos_lo=0.0, cos_hi=1.0, what=""):
    want_mask, want_pairs = vt.view_overlap(points, normals, rows, shape, depths, tol, min_cos,
                                            border, cos_lo, cos_hi)
    mask, pairs, _ = _overlap(points, normals, rows, shape, depths, tol, min_cos, border, cos_lo,
                              cos_hi)
    assert mask.dtype == want_mask.dtype == np.uint64
    differ = mask != want_mask
    assert not differ.any(), (what, "visible", int(differ.sum()), np.flatnonzero(differ)[:5],
                              mask[differ][:3], want_mask[differ][:3])
    assert np.array_equal(pairs, want_pairs), (what, "pairs", np.argwhere(pairs != want_pairs)[:5],
                                               pairs[pairs != want_pairs][:5],
                                               want_pairs[pairs != want_pairs][:5])
    return want_mask, want_pairs


def _gain(masks, V, chosen, redundancy):
    """rn_view_gain on a gain PAD entries longer than V + 1 and prefilled -> what was ADDED."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = _ctx()
    masks = np.ascontiguousarray(masks, np.uint64)
    d_masks = cuda(masks.view(np.int64))
    gain = torch.full((V + 1 + PAD,), GAIN_FILL, dtype=torch.int64, device="cuda")
    chosen = int(chosen) & 0xFFFFFFFFFFFFFFFF
    as_int64 = chosen - (1 << 64) if chosen >> 63 else chosen
    ctx._check(ctx.lib.rn_view_gain(ctx._h, len(masks), _ptr(d_masks), V, as_int64,
                                    int(redundancy), _ptr(gain), _stream()))
    assert_untouched(gain, V + 1, np.int64(GAIN_FILL), "gain")
    return gain.cpu().numpy()[:V + 1] - GAIN_FILL


# ------------------------------------------------------------------------------ a. the sizes
@pytest.fixture(scope="module")
def ring():
    cams, rows, points, shape = vt.ring_scene()
    normals = np.tile([0.0, 0.0, 1.0], (len(points), 1))
    normals[::7] = [0.3, -0.2, -1.0]                    # some face away
    normals[::11] = 0.0                                 # some face everything
    normals[5::13] = [2.0, 0.5, 0.4]                    # some are tilted, and not unit
    depths = vt.analytic_depths(cams, *shape)
    depths[:, 4:9, 10:20] *= F(0.5)                     # an occluder in every view
    depths[2, 12, 16], depths[3, 11, 15], depths[4, 12, 15] = 0.0, np.nan, -1.0
    return dict(cams=cams, rows=rows, points=points, shape=shape, normals=normals, depths=depths,
                band=vt.cosines(2.0, 45.0))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_masks_and_the_pairs_are_the_restatement_integer_for_integer(ring, n):
    """The ring of eight views over n points spread over the plane's grid, a NaN and two infinite
    points among them from n = 63 on; with and without normals, with and without depth maps."""
    total = len(ring["points"])
    take = (total // 2 + np.arange(n) * (total // n)) % total       # the grid's centre first
    points, normals = ring["points"][take].copy(), ring["normals"][take]
    assert len(points) == n == len(set(take.tolist()))
    if n >= 63:
        points[5, 0], points[17, 1], points[40, 2] = np.nan, np.inf, -np.inf
    cos_lo, cos_hi = ring["band"]
    bits = shared = 0
    for with_normals in (False, True):
        for with_depths in (False, True):
            for min_cos, border in ((0.0, 0.0), (0.3, 2.5)):
                mask, pairs = _held_to_the_truth(
                    points, normals if with_normals else None, ring["rows"], ring["shape"],
                    ring["depths"] if with_depths else None, 0.05, min_cos, border, cos_lo, cos_hi,
                    "ring, n %d, normals %s, depths %s" % (n, with_normals, with_depths))
                bits += int(vt.popcount(mask).sum())
                shared += int(np.triu(pairs, 1).sum())
                if n >= 63:
                    assert not mask[[5, 17, 40]].any()
    print("n %d: %d bits, %d shared points over the 8 settings" % (n, bits, shared))
    assert bits > 0 and (shared > 0 or n == 1)


def test_more_tiles_than_blocks_the_stride_loop_runs():
    """n one above the block cap times the block size, V = 3: block 0 takes a second tile, of one
    point, in which 255 lanes have no point."""
    n = CAP + 1
    rng = np.random.default_rng(2)
    points = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-0.2, 0.2, n)], 1)
    points[-1] = [0.1, 0.1, 0.0]                        # the last point is seen by all three
    cams = [PlaneCamera(-0.5, 0.0, 3.0, 20.0, 15.5, 11.5), PlaneCamera(0.5, 0.1, 3.0, 20.0, 15.5, 11.5),
            PlaneCamera(0.0, -0.6, 3.2, 20.0, 15.5, 11.5)]
    mask, pairs = _held_to_the_truth(points, None, pack_cameras(cams), (24, 32), None, cos_lo=0.9,
                                     cos_hi=0.999, what="n above the cap")
    assert mask[-1] == 7 and pairs[0, 0] > 1000 and pairs[0, 1] > 0


# ------------------------------------------------------------------------------ b. the views
@pytest.mark.parametrize("V", [1, 2, 3, 33, 64])
def test_one_to_sixty_four_views(V):
    """V cameras on a small ring, all over the same patch of the plane: bit V - 1 is set, and the
    last counter of the table -- pair (V - 1, V - 1) -- and the last off-diagonal one are used."""
    H, W = 13, 17
    cams = [PlaneCamera(0.4 * np.cos(0.7 * v), 0.4 * np.sin(0.7 * v), 3.0 + 0.01 * v, 20.0,
                        (W - 1) / 2.0, (H - 1) / 2.0) for v in range(V)]
    rows = pack_cameras(cams)
    g = np.linspace(-1.6, 1.6, 17)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    points = np.stack([gx.reshape(-1), gy.reshape(-1), 0.05 * np.sin(3 * gx.reshape(-1))], 1)
    depths = vt.analytic_depths(cams, H, W)
    for dm in (None, depths):
        mask, pairs = _held_to_the_truth(points, None, rows, (H, W), dm, 0.2, 0.0, 0.0,
                                         *vt.cosines(1.0, 30.0), what="V %d" % V)
        assert vt.bit(mask, V - 1).any() and pairs[V - 1, V - 1] > 0
        assert not (mask & ~vt.low_bits(V)).any()
        if V > 1:
            assert pairs[V - 2, V - 1] > 0


def test_a_wavefront_in_which_no_lane_or_one_lane_sees_a_view():
    """Views 0 and 1 over the origin, views 2 and 3 over (20, 0): the first wavefront's points
    are all under 0 and 1; in the second, lane 70 alone is under 2 and 3; in the third, lane 130
    alone is under 0 and 1 and the rest are nowhere."""
    cams = [PlaneCamera(-0.2, 0.0, 3.0, 20.0, 15.5, 11.5), PlaneCamera(0.2, 0.0, 3.0, 20.0, 15.5, 11.5),
            PlaneCamera(19.8, 0.0, 3.0, 20.0, 15.5, 11.5), PlaneCamera(20.2, 0.0, 3.0, 20.0, 15.5, 11.5)]
    rng = np.random.default_rng(4)
    n = 192
    points = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.zeros(n)], 1)
    points[70] = [20.0, 0.1, 0.0]
    points[128:] = [100.0, 100.0, 0.0]
    points[130] = [0.05, 0.0, 0.0]
    mask, pairs = _held_to_the_truth(points, None, pack_cameras(cams), (24, 32), None,
                                     cos_lo=0.5, cos_hi=1.0, what="sparse wavefronts")
    assert (mask[:64] == 3).all() and mask[70] == 12 and (np.delete(mask[64:128], 6) == 3).all()
    assert mask[130] == 3 and not np.delete(mask[128:], 2).any()
    assert pairs.tolist() == [[128, 128, 0, 0], [0, 128, 0, 0], [0, 0, 1, 1], [0, 0, 0, 1]]


def test_the_two_exact_cases_of_the_band():
    origin = np.zeros((1, 3))

    def shared(c0, c1, cos_lo, cos_hi):
        rows = pack_cameras([PlaneCamera(*c0, 8.0, 15.5, 11.5), PlaneCamera(*c1, 8.0, 15.5, 11.5)])
        mask, pairs = _held_to_the_truth(origin, None, rows, (24, 32), None, cos_lo=cos_lo,
                                         cos_hi=cos_hi, what="band")
        assert mask.tolist() == [3] and pairs[0, 0] == pairs[1, 1] == 1
        return int(pairs[0, 1])

    half = ((1.0, 0.0, 1.0), (0.0, 1.0, 1.0))
    assert shared(*half, 0.5, 1.0) == 1 and shared(*half, float(np.nextafter(0.5, 1.0)), 1.0) == 0
    assert shared(*half, 0.0, 0.5) == 1 and shared(*half, 0.0, float(np.nextafter(0.5, 0.0))) == 0
    # 4/5 in exact arithmetic, but 0.8 * 0.8 * 400 = 256.00000000000006 > 256: not at cos_lo = 0.8
    fifths = ((0.0, 0.0, 4.0), (3.0, 0.0, 4.0))
    assert shared(*fifths, 0.8, 1.0) == 0 and shared(*fifths, float(np.nextafter(0.8, 0.0)), 1.0) == 1


def test_two_calls_over_two_halves_add_up_to_the_call_over_the_whole(ring):
    points, rows, shape = ring["points"][:1000], ring["rows"], ring["shape"]
    cos_lo, cos_hi = ring["band"]
    args = (ring["rows"], shape, ring["depths"], 0.05, 0.0, 0.0, cos_lo, cos_hi)
    whole_mask, whole, _ = _overlap(points, ring["normals"][:1000], *args)
    first_mask, first, device_pairs = _overlap(points[:437], ring["normals"][:437], *args)
    second_mask, second, _ = _overlap(points[437:], ring["normals"][437:1000], *args,
                                      pairs=device_pairs)
    assert np.array_equal(first + second, whole) and np.triu(whole, 1).any()
    assert np.array_equal(np.concatenate([first_mask, second_mask]), whole_mask)
    assert np.array_equal(device_pairs.cpu().numpy()[:len(rows)] - PAIRS_FILL, whole)


# ------------------------------------------------------------------------------ c. the gains
def _random_masks(n, V, seed):
    rng = np.random.default_rng(seed)
    bits = rng.random((n, 64)) < rng.uniform(0.02, 0.6, (n, 1))     # sparse to dense rows
    bits[::17] = False
    bits[3::29] = True
    masks = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    return masks                                        # (bits at V and above are garbage on purpose)


@pytest.mark.parametrize("V,n", [(64, 1000), (33, 257), (3, 65), (1, 1), (3, CAP + 1)])
def test_the_gains_are_the_restatement(V, n):
    masks = _random_masks(n, V, V + n)
    some = 0
    for chosen in (0, 1, 1 << 63, (1 << 64) - 1, 1 << (V - 1), 0x5555555555555555):
        for redundancy in (1, 2, 64):
            want = vt.gain(masks, V, chosen, redundancy)
            got = _gain(masks, V, chosen, redundancy)
            assert np.array_equal(got, want), (V, n, hex(chosen), redundancy, got, want)
            for v in range(V):
                assert not ((chosen >> v) & 1 and got[v])
            some += int(got.sum())
    assert some > 0
    if V == 64:
        assert vt.gain(masks, 64, 0, 1)[63] > 0 and vt.gain(masks, 64, 1 << 63, 1)[63] == 0


# ------------------------------------------------------------------------------ d. the package
def test_cover_and_neighbors_on_the_ring_are_the_truths(ring):
    from raynet_amd.view_selection import ViewOverlap, view_overlap
    got = view_overlap(ring["points"], ring["cams"], ring["shape"], min_angle=2.0, max_angle=45.0)
    assert isinstance(got, ViewOverlap) and got.visible.dtype == np.uint64
    mask, pairs = vt.view_overlap(ring["points"], None, ring["rows"], ring["shape"], None, 0.0, 0.0,
                                  0.0, *ring["band"])
    assert np.array_equal(got.visible, mask) and np.array_equal(got.pairs, vt.symmetric(pairs))
    for i in range(8):
        assert got.neighbors(i, 2) == vt.neighbors(got.pairs, i, 2)
        assert sorted(got.neighbors(i, 2)) == sorted([(i - 1) % 8, (i + 1) % 8])
    for k, redundancy in ((8, 1), (3, 1), (8, 2), (8, 8)):
        assert got.cover(k, redundancy) == vt.cover(mask, 8, k, redundancy), (k, redundancy)
    order = got.cover(8, 1)[0]
    assert (order[1] - order[0]) % 8 == 4
    assert got.cover(8, 1, candidates=[6, 2, 3]) == vt.cover(mask, 8, 8, 1, candidates=[6, 2, 3])
    # normals, depth maps and a tensor of float32 points go through as well
    import torch
    got = view_overlap(torch.from_numpy(ring["points"].astype(F)), ring["cams"], ring["shape"],
                       normals=ring["normals"], depth_maps=list(ring["depths"]), tol=0.05,
                       min_cos=0.3, border=1.0)
    mask, pairs = vt.view_overlap(ring["points"].astype(F).astype(D), ring["normals"], ring["rows"],
                                  ring["shape"], ring["depths"], 0.05, 0.3, 1.0, *ring["band"])
    assert np.array_equal(got.visible, mask) and np.array_equal(got.pairs, vt.symmetric(pairs))


def test_best_frames_on_the_two_sphere_mesh():
    import mesh_harness as h
    from raynet_amd.common.scene import Image, Scene
    from raynet_amd.fusion import fuse_depth_maps
    bbox, cams, H, W, grid, _, _, gt_maps = h.two_sphere_maps()
    mesh = fuse_depth_maps(gt_maps, cams, bbox, grid, trunc=0.25).mesh()
    assert not mesh.empty and mesh.normals is None
    scene = Scene([Image(np.zeros((H, W, 3), F), cam) for cam in cams], bbox=bbox)
    tol = float(np.sqrt(((2.0 / np.asarray(grid)) ** 2).sum()))
    frames, gains, short = mesh.best_frames(scene, [2, 0, 1], 3, tol, return_stats=True)
    assert mesh.normals is not None                     # computed on the way
    caster = mesh.raycaster()
    order = [2, 0, 1]
    depths = np.stack([caster.depth_map(cams[i], H, W).cpu().numpy() for i in order])
    mask = vt.visible(mesh.vertices.astype(D), mesh.normals.astype(D),
                      pack_cameras([cams[i] for i in order]), (H, W), depths, tol, 0.0, 0.0)
    want = vt.cover(mask, 3, 3, 1)
    assert (frames, gains, short) == ([order[v] for v in want[0]], want[1], want[2])
    assert len(frames) >= 2 and gains[0] >= gains[-1] > 0 and short < len(mesh.vertices)
    assert mesh.best_frames(scene, [2, 0, 1], 1, tol) == frames[:1]
    want2 = vt.cover(mask, 3, 3, 2)
    assert mesh.best_frames(scene, [2, 0, 1], 3, tol, redundancy=2) == [order[v] for v in want2[0]]
    with pytest.raises(ValueError, match="candidate frames"):
        mesh.best_frames(scene, list(range(65)), 3, tol)


def test_select_views_on_the_command_line(tmp_path, capsys, monkeypatch):
    """fuse_depth_maps --gt --color on the two-sphere scene: with --select_views 2 all three maps
    are fused (the surface is the same) but the colours come from the two frames best_frames
    chose, which are printed; select_views writes the matrix, the neighbours and the cover."""
    import json
    import os
    import re
    import mesh_harness as h
    from raynet_amd.scripts import fuse_depth_maps, select_views
    from raynet_amd.volume import SurfaceMesh
    bbox, cams, H, W, grid, _, _, gt_maps = h.two_sphere_maps()
    scene_dir, preds = str(tmp_path / "scene"), str(tmp_path / "predictions")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    os.makedirs(preds)
    asked = []
    colorize, best_frames = SurfaceMesh.colorize, SurfaceMesh.best_frames

    def spy_colorize(self, scene, frame_idxs, **kw):
        asked.append(("colorize", list(frame_idxs), kw["tol"]))
        return colorize(self, scene, frame_idxs, **kw)

    def spy_best_frames(self, scene, frame_idxs, k, tol, **kw):
        got = best_frames(self, scene, frame_idxs, k, tol, **kw)
        asked.append(("best_frames", list(frame_idxs), k, tol, got))
        return got

    monkeypatch.setattr(SurfaceMesh, "colorize", spy_colorize)
    monkeypatch.setattr(SurfaceMesh, "best_frames", spy_best_frames)
    flags = ["--gt", "--truncation", "0.25", "--start_end", "0,3", "--grid_shape", "18,22,14",
             "--color"]
    every, two = str(tmp_path / "every.ply"), str(tmp_path / "two.ply")
    assert fuse_depth_maps.main([scene_dir, preds, every] + flags) == 0
    assert "--select_views" not in capsys.readouterr().out
    assert [a[:2] for a in asked] == [("colorize", [0, 1, 2])]
    del asked[:]
    assert fuse_depth_maps.main([scene_dir, preds, two] + flags + ["--select_views", "2"]) == 0
    printed = capsys.readouterr().out
    (_, candidates, k, tol, (chosen, gains, short)), (_, coloured, colour_tol) = asked
    assert candidates == [0, 1, 2] and k == 2 and len(chosen) == 2 and coloured == chosen
    assert tol == colour_tol                             # the tolerance the colour step is given
    a, b = SurfaceMesh.load_ply(every), SurfaceMesh.load_ply(two)
    assert np.array_equal(a.vertices, b.vertices) and np.array_equal(a.faces, b.faces)
    assert b.colors is not None and not np.array_equal(a.colors, b.colors)
    m = re.search(r"--select_views: frames ([\d,]+) of 3 candidates; ([\d.]+) of the (\d+) vertices",
                  printed)
    assert m and [int(x) for x in m.group(1).split(",")] == chosen
    assert int(m.group(3)) == len(b.vertices) and m.group(2) == "%.4f" % (short / len(b.vertices))
    # select_views: the matrix is symmetric, every frame lists the other two, the cover is
    # best_frames' on the written mesh
    out = str(tmp_path / "views.json")
    assert select_views.main([scene_dir, out, "--start_end", "0,3", "--neighbors", "4", "--proxy_grid",
                              "9,11,7", "--mesh", two, "--cover", "2", "--depth_tolerance",
                              repr(tol)]) == 0
    got = json.load(open(out))
    pairs = np.array(got["pairs"])
    assert got["frames"] == [0, 1, 2] and pairs.shape == (3, 3) and np.array_equal(pairs, pairs.T)
    assert (np.diag(pairs) > 0).all()
    assert all(sorted(got["neighbors"][str(i)]) == sorted({0, 1, 2} - {i}) for i in range(3))
    assert got["cover"]["frames"] == chosen and got["cover"]["gains"] == gains
    assert got["cover"]["short"] == short and got["cover"]["vertices"] == len(b.vertices)


# ------------------------------------------------------------------------------ e. refusals
def test_bad_arguments_are_refused_before_any_launch(ring):
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = _ctx()
    last = ctx.lib.rn_last_error
    null = ctypes.c_void_p(0)
    INVALID = -1
    n, V = 65, 8
    dpts = cuda(ring["points"][:n].T, D)
    dnrm = cuda(ring["normals"][:n].T, D)
    dcam, ddep = cuda(ring["rows"], D), cuda(ring["depths"], F)
    visible = torch.full((n,), VISIBLE_FILL, dtype=torch.int64, device="cuda")
    pairs = torch.full((V, V), PAIRS_FILL, dtype=torch.int64, device="cuda")
    gain = torch.full((V + 1,), GAIN_FILL, dtype=torch.int64, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((visible == VISIBLE_FILL).all() and (pairs == PAIRS_FILL).all() and
                    (gain == GAIN_FILL).all())

    #       0  1           2           3  4           5   6   7           8    9    10   11   12
    good = [n, _ptr(dpts), _ptr(dnrm), V, _ptr(dcam), 24, 32, _ptr(ddep), 0.1, 0.2, 0.0, 0.7, 0.99,
            _ptr(visible), _ptr(pairs)]
    nan, inf = float("nan"), float("inf")
    bad = [(0, -1), (0, (1 << 38) + 1), (3, 0), (3, -1), (3, 65), (5, 0), (6, 0), (5, -24),
           (8, -0.1), (8, nan), (8, inf), (9, -0.2), (9, nan), (9, inf), (10, -1.0), (10, nan),
           (10, inf), (11, -0.1), (11, nan), (11, 0.995), (12, 1.5), (12, nan), (12, 0.5)] + \
          [(k, null) for k in (1, 4, 13, 14)]
    for at_, value in bad:
        args = list(good)
        args[at_] = value
        assert ctx.lib.rn_view_overlap(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_view_overlap" in last(ctx._h)
    assert untouched()
    # n == 0 returns cleanly, whatever the pointers, and writes nothing
    args = [0, null, null, V, null, 24, 32, null, 0.1, 0.2, 0.0, 0.7, 0.99, null, null]
    assert ctx.lib.rn_view_overlap(ctx._h, *args, _stream()) == _lib.RN_OK
    args = list(good)
    args[0] = 0
    assert ctx.lib.rn_view_overlap(ctx._h, *args, _stream()) == _lib.RN_OK
    # rn_view_gain
    #        0  1              2  3  4  5
    good_g = [n, _ptr(visible), V, 0, 1, _ptr(gain)]
    for at_, value in [(0, -1), (0, (1 << 38) + 1), (2, 0), (2, 65), (2, -3), (4, 0), (4, 65),
                       (4, -1), (1, null), (5, null)]:
        args = list(good_g)
        args[at_] = value
        assert ctx.lib.rn_view_gain(ctx._h, *args, _stream()) == INVALID, (at_, value)
        assert b"rn_view_gain" in last(ctx._h)
    assert ctx.lib.rn_view_gain(ctx._h, 0, null, V, -1, 1, null, _stream()) == _lib.RN_OK
    assert untouched()
    # the wrappers: the entry's name on a refusal, and tensors that are not what the kernels read
    with pytest.raises(_lib.RaynetHipError, match="rn_view_overlap"):
        ctx.view_overlap(dpts, None, dcam, (24, 32), None, -1.0, 0.0, 0.0, 0.7, 0.99)
    call = dict(points=dpts, normals=dnrm, cameras=dcam, image_shape=(24, 32), depths=ddep, tol=0.1,
                min_cos=0.2, border=0.0, cos_lo=0.7, cos_hi=0.99)
    for kw, match in [
            (dict(points=dpts.float()), "points"), (dict(points=dpts.t().contiguous()), "points"),
            (dict(points=dpts[:, ::2]), "points"), (dict(points=dpts.cpu()), "points"),
            (dict(normals=dnrm.float()), "normals"), (dict(normals=dnrm[:, :-1]), "normals"),
            (dict(cameras=dcam.float()), "cameras"), (dict(cameras=dcam[:, :14]), "cameras"),
            (dict(cameras=dcam[:1].expand(65, 15).contiguous()), "cameras"),
            (dict(depths=ddep.double()), "depths"), (dict(depths=ddep[:7]), "depths"),
            (dict(depths=ddep[:, :, ::2]), "depths"), (dict(image_shape=(24, 31)), "depths"),
            (dict(visible=visible[:-1]), "visible"), (dict(visible=visible.int()), "visible"),
            (dict(pairs=pairs[:7]), "pairs"), (dict(pairs=pairs.int()), "pairs")]:
        args = dict(call)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ctx.view_overlap(**args)
    for kw, match in [(dict(V=0), "V"), (dict(V=65), "V"), (dict(redundancy=0), "redundancy"),
                      (dict(redundancy=65), "redundancy"), (dict(visible=visible.int()), "visible"),
                      (dict(visible=visible.cpu()), "visible"), (dict(visible=visible[::2]), "visible"),
                      (dict(gain=gain[:V]), "gain"), (dict(gain=gain.int()), "gain")]:
        args = dict(visible=visible, V=V, chosen=0, redundancy=1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ctx.view_gain(**args)
    assert untouched()
    # ... and what is accepted writes all n masks, adds to the given matrix and to the given gain
    out = ctx.view_overlap(**call, visible=visible, pairs=pairs)
    assert out[0] is visible and out[1] is pairs
    want_mask, want_pairs = vt.view_overlap(ring["points"][:n], ring["normals"][:n], ring["rows"],
                                            (24, 32), ring["depths"], 0.1, 0.2, 0.0, 0.7, 0.99)
    assert np.array_equal(visible.cpu().numpy().view(np.uint64), want_mask)
    assert np.array_equal(pairs.cpu().numpy() - PAIRS_FILL, want_pairs)
    assert ctx.view_gain(visible, V, 0b101, 2, gain) is gain
    assert np.array_equal(gain.cpu().numpy() - GAIN_FILL, vt.gain(want_mask, V, 0b101, 2))
    fresh = ctx.view_gain(visible, V, -1, 1)
    assert np.array_equal(fresh.cpu().numpy(), vt.gain(want_mask, V, -1, 1))
    none = ctx.view_overlap(torch.empty((3, 0), dtype=torch.float64, device="cuda"), None, dcam,
                            (24, 32), None, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert tuple(none[0].shape) == (0,) and not none[1].any()
