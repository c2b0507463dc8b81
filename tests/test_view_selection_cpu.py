"""View selection, the host side (no GPU): the two entries in the header and the ctypes table, the
argument checks, launch geometry and predicates of the launchers
(raynet_amd/csrc/raynet_overlap_args.h) as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter -- the shape of
the kernel file, the ordering rules of ViewOverlap.neighbors and .cover with the gain call stubbed
by the truth, what the package refuses before it asks for a device, what it does without one, and
the parser errors of the new flags."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import view_selection_truth as vt
from conftest import REPO
from host_program import run_host_program

CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_launcher_checks_under_sanitizers(tmp_path):
    run_host_program("overlap", tmp_path)


def test_the_entries_are_declared_and_bound_with_matching_types():
    """(The types of every entry, these included: tests/test_abi.py.)"""
    from raynet_amd import _lib
    assert abi_header.prototype("rn_view_overlap") == ("int", [
        "rn_ctx *ctx", "int64_t n", "const double *points", "const double *normals", "int32_t V",
        "const double *cameras", "int32_t H", "int32_t W", "const float *depths", "double tol",
        "double min_cos", "double border", "double cos_lo", "double cos_hi", "uint64_t *visible",
        "int64_t *pairs", "void *stream"])
    assert abi_header.prototype("rn_view_gain") == ("int", [
        "rn_ctx *ctx", "int64_t n", "const uint64_t *visible", "int32_t V", "int64_t chosen",
        "int32_t redundancy", "int64_t *gain", "void *stream"])
    lib = ctypes.CDLL(_lib.build())
    assert hasattr(lib, "rn_view_overlap") and hasattr(lib, "rn_view_gain")
    assert len(_lib.SIGNATURES["rn_view_overlap"]) == 17 and len(_lib.SIGNATURES["rn_view_gain"]) == 8


def test_the_launchers_and_the_kernels_use_these_checks():
    """raynet_overlap.inl decides on the header's verdicts and sees, shares and counts with its
    functions; the file is plain HIP with integer atomics only, no inline assembly and no square
    root; no lane leaves before the ballots."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_overlap.inl")).read()
    code = re.sub(r"//.*", "", src)
    for word in ("asm", "sqrt", "float *pairs", "double *pairs", "atomicAdd((float", "h2", "cam["):
        assert word not in code, word
    assert "return;" not in code                        # a lane without a point stays in the ballots
    assert code.count("rn_overlap::overlap_args(") == 1 and code.count("rn_overlap::gain_args(") == 1
    assert code.count("if (verdict == rn_overlap::INVALID)") == 2
    assert code.count("if (verdict == rn_overlap::EMPTY) return RN_OK;") == 2
    for use in ("rn_overlap::sees(", "rn_overlap::to_centre(", "rn_overlap::shares(",
                "rn_overlap::is_short(", "rn_overlap::point_in(", "rn_overlap::coord_index(",
                "rn_overlap::pair_index(", "rn_overlap::matrix_index(", "rn_overlap::tiles(",
                "rn_overlap::blocks(", "rn_overlap::low_bits(", "__ballot(", "__popcll("):
        assert use in code, use
    assert "__shared__ uint32_t counts[rn_overlap::MAX_PAIRS];" in code
    # every global atomic adds a 64-bit integer
    assert len(re.findall(r"atomicAdd\(&a\.(pairs|gain)\[", code)) == 2
    assert "unsigned long long *pairs;" in code and "unsigned long long *gain;" in code
    header = open(os.path.join(CSRC, "raynet_overlap_args.h")).read()
    plain = re.sub(r"//.*", "", header)
    assert "hip" not in plain.lower() and "sqrt" not in plain and "__device__" not in plain
    assert "rn_view::project(" in plain and "static_assert(block_points_max(MAX_POINTS)" in plain
    for f in ("raynet_overlap.inl", "raynet_overlap_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
        assert os.path.join(CSRC, f) in _lib.sources(), f
    assert '#include "raynet_overlap.inl"' in open(os.path.join(CSRC, "raynet_hip.hip")).read()


# ------------------------------------------------------------------------------ orderings
def _stubbed(masks, V):
    """A ViewOverlap over hand-made masks whose gain call is the truth's."""
    from raynet_amd.view_selection import ViewOverlap
    masks = np.asarray(masks, np.uint64)
    o = ViewOverlap(masks, np.zeros((V, V), np.int64))
    calls = []

    def gain(chosen, redundancy):
        calls.append((chosen, redundancy))
        return [int(g) for g in vt.gain(masks, V, chosen, redundancy)]

    o._gain = gain
    return o, calls


def test_neighbors_orders_a_row_of_the_matrix():
    from raynet_amd.view_selection import ViewOverlap
    upper = np.array([[9, 4, 0, 4, 7], [0, 9, 0, 0, 0], [0, 0, 9, 0, 0], [0, 0, 0, 9, 0],
                      [0, 0, 0, 0, 9]])
    o = ViewOverlap(np.zeros(1, np.uint64), vt.symmetric(upper))
    assert o.neighbors(0, 4) == [4, 1, 3, 2]            # the tie to the lower j, the 0 last
    assert o.neighbors(2, 4) == [0, 1, 3, 4]            # all 0: index order
    assert o.neighbors(0, 2) == [4, 1] and o.neighbors(0, 0) == [] and o.neighbors(0, 9) == [4, 1, 3, 2]
    for i in range(5):
        assert o.neighbors(i, 4) == vt.neighbors(o.pairs, i, 4)
    with pytest.raises(ValueError, match="i:"):
        o.neighbors(5, 1)
    with pytest.raises(ValueError, match="k:"):
        o.neighbors(0, -1)
    with pytest.raises(ValueError, match="pairs"):
        ViewOverlap(np.zeros(1, np.uint64), np.zeros((2, 3)))


def test_cover_is_the_greedy_loop_with_ties_to_the_lower_index():
    masks = [0b0001, 0b0011, 0b0111, 0b1000, 0b0000, 0b1111, 0b0110]
    o, calls = _stubbed(masks, 4)
    assert o.cover(4, 2) == ([0, 1, 2, 3], [4, 4, 1, 1], 3) == vt.cover(np.array(masks, np.uint64), 4, 4, 2)
    assert [c[0] for c in calls] == [0, 0b1, 0b11, 0b111, 0b1111]    # one gain call per pick, one last
    o, calls = _stubbed(masks, 4)
    # views 0 and 1 tie at 4: the lower wins; then nothing but view 3 adds anything (1000)
    assert o.cover(4, 1) == ([0, 1, 3], [4, 1, 1], 1)
    assert o.cover(1, 1) == ([0], [4], 3) and o.cover(0, 1) == ([], [], 7)
    assert o.cover(4, 1, candidates=[3, 2]) == ([2, 3], [3, 1], 3)
    assert o.cover(4, 1, candidates=[]) == ([], [], 7)
    for kw, match in ((dict(k=-1), "k:"), (dict(k=1, redundancy=0), "redundancy"),
                      (dict(k=1, redundancy=65), "redundancy"), (dict(k=1, candidates=[4]), "candidates"),
                      (dict(k=1, candidates=[-1]), "candidates")):
        with pytest.raises(ValueError, match=match):
            o.cover(**kw)
    # bit 63
    top = [1 << 63, (1 << 64) - 1, 0, (1 << 63) | 1]
    o, _ = _stubbed(top, 64)
    assert o.cover(64, 1) == ([63], [3], 1) == vt.cover(np.array(top, np.uint64), 64, 64, 1)


# ------------------------------------------------------------------------------ refusals
def _cams(V):
    return [vt.PlaneCamera(0.1 * v, 0.0, 3.0, 20.0, 15.5, 11.5) for v in range(V)]


def test_bad_inputs_raise_before_a_device_is_asked_for(monkeypatch):
    import torch
    from raynet_amd import view_selection as vs

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(vs, "_context", no_device)
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    pts, cams, shape = np.zeros((4, 3)), _cams(3), (24, 32)
    nan, inf = float("nan"), float("inf")
    bad = [(dict(points=np.zeros((3, 4))), "points"), (dict(points=np.zeros(3)), "points"),
           (dict(normals=np.zeros((5, 3))), "normals"), (dict(cameras=_cams(65)), "65 views"),
           (dict(cameras=[]), "0 views"), (dict(image_shape=(0, 32)), "image_shape"),
           (dict(depth_maps=[np.zeros(shape)] * 2), "depth_maps"),
           (dict(depth_maps=[np.zeros((24, 31))] * 3), "depth_maps"),
           (dict(tol=-1.0), "tol"), (dict(tol=nan), "tol"), (dict(min_cos=inf), "min_cos"),
           (dict(min_cos=-0.5), "min_cos"), (dict(border=nan), "border"), (dict(border=-1), "border"),
           (dict(min_angle=-1.0), "min_angle"), (dict(max_angle=91.0), "max_angle"),
           (dict(min_angle=50.0), "min_angle"), (dict(min_angle=nan), "min_angle"),
           (dict(max_angle=nan), "max_angle")]
    for kw, match in bad:
        call = dict(points=pts, cameras=cams, image_shape=shape)
        call.update(kw)
        with pytest.raises(ValueError, match=match):
            vs.view_overlap(**call)


def test_degrees_become_cosines_on_the_host():
    from raynet_amd.view_selection import band_cosines
    assert band_cosines(0.0, 90.0) == (0.0, 1.0)
    lo, hi = band_cosines(2.0, 45.0)
    assert (lo, hi) == vt.cosines(2.0, 45.0) and 0.0 < lo < hi < 1.0
    assert lo == float(np.cos(np.deg2rad(45.0))) and hi == float(np.cos(np.deg2rad(2.0)))
    assert band_cosines(30.0, 30.0)[0] == band_cosines(30.0, 30.0)[1]


def test_no_device_is_an_error_not_a_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from raynet_amd import _lib
    from raynet_amd.view_selection import ViewOverlap, view_overlap
    with pytest.raises(_lib.RaynetHipError, match="no GPU"):
        view_overlap(np.zeros((4, 3)), _cams(3), (24, 32))
    with pytest.raises(_lib.RaynetHipError, match="no GPU"):
        ViewOverlap(np.zeros(4, np.uint64), np.zeros((3, 3), np.int64)).cover(2)


def test_use_overlap_neighbors_refuses_sixty_five_images(monkeypatch):
    from raynet_amd import view_selection as vs
    from raynet_amd.common.scene import Image, Scene
    images = [Image(np.zeros((24, 32, 3), np.float32), cam) for cam in _cams(65)]
    scene = Scene(images, bbox=[-1, -1, -1, 1, 1, 1])
    with pytest.raises(ValueError, match='"distance"'):
        scene.use_overlap_neighbors()
    assert scene._get_neighbor_idxs(3, 2) == [2, 4]     # the scene is left as it was: file order
    # with a table the neighbours come from it, whatever the constructor's flag
    small = Scene(images[:5], bbox=[-1, -1, -1, 1, 1, 1], select_neighbors_based_on="distance")
    upper = np.array([[9, 4, 0, 4, 7], [0, 9, 1, 2, 3], [0, 0, 9, 0, 0], [0, 0, 0, 9, 5],
                      [0, 0, 0, 0, 9]])
    seen = {}

    def stub(points, cameras, image_shape, **kw):
        seen.update(n=len(points), V=len(cameras), shape=tuple(image_shape), kw=kw)
        return vs.ViewOverlap(np.zeros(1, np.uint64), vt.symmetric(upper))

    monkeypatch.setattr(vs, "view_overlap", stub)
    small.use_overlap_neighbors(grid_shape=(4, 3, 2), min_angle=1.0, max_angle=30.0)
    assert seen == dict(n=24, V=5, shape=(24, 32), kw=dict(min_angle=1.0, max_angle=30.0))
    assert small._get_neighbor_idxs(0, 3) == [4, 1, 3] and small._get_neighbor_idxs(1, 4) == [0, 4, 3, 2]
    assert small.view_indices_with_neighbors(3, 2) == [3, 4, 0]


# ------------------------------------------------------------------------------ the flags
def _error(main, argv, capsys, match):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2
    assert match in capsys.readouterr().err, match


def test_the_parser_errors_of_the_new_flags(tmp_path, capsys):
    from raynet_amd.scripts import forward_pass, fuse_depth_maps, render_mesh, render_volume
    from raynet_amd.scripts import select_views
    d, out = str(tmp_path), str(tmp_path / "out")
    fuse = lambda *more: ([d, d, out + ".ply"] + list(more))             # noqa: E731
    _error(fuse_depth_maps.main, fuse("--select_views", "4"), capsys, "--select_views goes with")
    _error(fuse_depth_maps.main, fuse("--color", "--select_views", "0"), capsys, "1..32")
    _error(fuse_depth_maps.main, fuse("--color", "--select_views", "33"), capsys, "1..32")
    _error(fuse_depth_maps.main, fuse("--color", "--view_redundancy", "2"), capsys,
           "--view_redundancy goes with --select_views")
    _error(fuse_depth_maps.main, fuse("--color", "--select_views", "4", "--view_redundancy", "0"),
           capsys, "--view_redundancy takes 1..64")
    _error(fuse_depth_maps.main, fuse("--texture", "4", "--select_views", "4", "--view_redundancy",
                                      "65"), capsys, "--view_redundancy takes 1..64")
    occ = str(tmp_path / "occupancy.npz")
    _error(render_volume.main, [d, occ, out, "--select_views", "4"], capsys, "--select_views goes with")
    _error(render_volume.main, [d, occ, out, "--mesh", out + ".ply", "--color", "--select_views",
                                "40"], capsys, "1..32")
    _error(render_mesh.main, [d, out + ".ply", out, "--select_views", "4"], capsys,
           "--select_views goes with")
    _error(render_mesh.main, [d, out + ".ply", out, "--texture", "4", "--view_redundancy", "2"],
           capsys, "--view_redundancy goes with")
    _error(forward_pass.main, [d, out, "--neighbors_by_overlap", "--select_neighbors_based_on",
                               "distance"], capsys, "--neighbors_by_overlap replaces")
    _error(select_views.main, [d, out + ".json", "--min_angle", "50"], capsys, "--min_angle")
    _error(select_views.main, [d, out + ".json", "--max_angle", "91"], capsys, "--max_angle")
    _error(select_views.main, [d, out + ".json", "--view_redundancy", "0"], capsys, "--view_redundancy")
    _error(select_views.main, [d, out + ".json", "--proxy_grid", "4,4"], capsys, "--proxy_grid")
    _error(select_views.main, [d, out + ".json", "--mesh", out + ".ply"], capsys, "no such file")
    # the defaults: nothing is asked for
    for script in (fuse_depth_maps, render_volume, render_mesh):
        args = script.build_parser().parse_args([d, d, d])
        assert args.select_views is None and args.view_redundancy is None
    assert forward_pass.build_parser().parse_args([d, d]).neighbors_by_overlap is False


def test_more_than_sixty_four_candidates_is_a_parser_error():
    import argparse
    from raynet_amd.scripts import texture_flags, view_flags

    class Stop(Exception):
        pass

    class Parser(object):
        def error(self, message):
            raise Stop(message)

    args = argparse.Namespace(select_views=8, view_redundancy=None, texture=4, color=True)
    view_flags.check(Parser(), args)
    view_flags.check_candidates(Parser(), args, list(range(64)))
    with pytest.raises(Stop, match="65 candidate frames, at most 64"):
        view_flags.check_candidates(Parser(), args, list(range(65)))
    # without the flag the frames go through as they are, and the 32-frame errors are the old ones
    args.select_views = None
    assert view_flags.choose(Parser(), args, None, None, [3, 1, 2], 0.1) == [3, 1, 2]
    view_flags.check_candidates(Parser(), args, list(range(65)))
    with pytest.raises(Stop, match="at most 32"):
        texture_flags.check_frames(Parser(), args, list(range(33)))
    # with it, the chosen frames are best_frames', printed

    class Mesh(object):
        empty, vertices = False, np.zeros((10, 3))

        def best_frames(self, scene, frames, k, tol, redundancy=1, return_stats=False):
            self.asked = (frames, k, tol, redundancy, return_stats)
            return [frames[2], frames[0]], [6, 3], 1

    args.select_views, args.view_redundancy, mesh = 2, 3, Mesh()
    assert view_flags.choose(Parser(), args, mesh, None, [5, 6, 7], 0.25) == [7, 5]
    assert mesh.asked == ([5, 6, 7], 2, 0.25, 3, True)
    with pytest.raises(Stop, match="--start_end selects no frame"):
        view_flags.choose(Parser(), args, mesh, None, [], 0.25)
