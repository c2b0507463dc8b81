"""The cross-view check, the host side (no GPU): the entry in the header and the ctypes table, the
argument checks, index arithmetic and per-view verdict of the launcher
(raynet_amd/csrc/raynet_consistency_args.h) as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter -- the shape of
the kernel file, DepthConsistency's counts and keep rule against the truth's, and what the package
does without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import consistency_truth as ct
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_launcher_checks_under_sanitizers(tmp_path):
    run_host_program("consistency", tmp_path)


def test_the_launcher_and_the_kernel_use_these_checks():
    """raynet_consistency.inl decides on the header's verdict, finds its point, addresses the
    arrays and classifies with its functions; the file is plain HIP without LDS, atomics or a
    square root, and its projection is the shared header's."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_consistency.inl")).read()
    code = re.sub(r"//.*", "", src)
    for word in ("asm", "__shared__", "atomic", "sqrt", "__syncthreads", "h2", "cam["):
        assert word not in code, word
    assert code.count("for (") == 1                     # the view loop is the only loop
    assert code.count("rn_consistency::points_args(") == 1
    assert "if (verdict == rn_consistency::INVALID)" in code
    assert "if (verdict == rn_consistency::EMPTY) return RN_OK;" in code
    for use in ("rn_consistency::point_in(", "rn_consistency::coord_index(",
                "rn_consistency::map_index(", "rn_consistency::pixel_in(",
                "rn_consistency::blocks(", "rn_consistency::classify("):
        assert use in code, use
    assert code.count("rn_view::project(") == 1
    # the one load of a map goes through the guarded pixel index, the points through coord_index
    assert re.findall(r"a\.depths\[(\w+)\]", code) == ["pixel"]
    assert len(re.findall(r"a\.points\[rn_consistency::coord_index\(", code)) == 3
    assert len(re.findall(r"a\.points\[", code)) == 3
    header = open(os.path.join(CSRC, "raynet_consistency_args.h")).read()
    plain = re.sub(r"//.*", "", header)
    assert "hip" not in plain.lower() and "sqrt" not in plain and "__device__" not in plain
    for f in ("raynet_consistency.inl", "raynet_consistency_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
        assert os.path.join(CSRC, f) in _lib.sources(), f
    assert '#include "raynet_consistency.inl"' in open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert "using rn_view::CAMERA_DOUBLES, rn_view::map_index, rn_view::pixel_in;" in header


def test_the_entry_is_declared_and_bound_with_matching_types():
    """(The types of every entry, this one included: tests/test_abi.py.)"""
    from raynet_amd import _lib
    assert abi_header.prototype("rn_points_consistency") == ("int", [
        "rn_ctx *ctx", "int64_t n", "const double *points", "int32_t V", "const double *cameras",
        "int32_t H", "int32_t W", "const float *depths", "int32_t exclude", "double tol_abs",
        "double tol_rel", "double border", "uint32_t *seen", "uint32_t *agree",
        "uint32_t *violate", "float *residual", "void *stream"])
    assert hasattr(ctypes.CDLL(_lib.build()), "rn_points_consistency")


def test_counts_keep_and_filtered_are_the_truths():
    from raynet_amd.consistency import DepthConsistency, popcount
    rng = np.random.default_rng(5)
    shape = (6, 7)
    seen = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    seen[0, :3] = [0, 0xFFFFFFFF, 0x80000000]
    agree = seen & rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    violate = seen & ~agree & rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    agree[1, :4] = [3, 1, 3, 0x80000001]
    violate[1, :4] = [0, 0, 4, 0]
    depth = rng.uniform(1, 3, shape).astype(F)
    depth[2, :4] = [0, -1, np.nan, np.inf]
    agree[2, :4], violate[2, :4] = 0xFF, 0
    with np.errstate(invalid="ignore"):
        measured = (depth > 0) & (depth < np.inf)
    c = DepthConsistency(seen, agree, violate, np.zeros(shape, F), measured)
    for got, mask in ((c.seen_count, seen), (c.agree_count, agree), (c.violate_count, violate)):
        assert got.dtype == np.uint8 and got.shape == shape
        assert np.array_equal(got, ct.popcount(mask))
    assert popcount(np.array([0, 1, 0x80000001, 0xFFFFFFFF], np.uint32)).tolist() == [0, 1, 2, 32]
    for min_views, max_violations in ((2, 0), (1, 0), (0, 0), (3, 2), (1, 32)):
        want = ct.keep(depth, agree, violate, min_views, max_violations)
        assert np.array_equal(c.keep(min_views, max_violations), want)
        out = c.filtered(depth, min_views, max_violations)
        assert out.dtype == F and np.array_equal(out[want], depth[want]) and (out[~want] == 0).all()
    assert c.keep()[1, :4].tolist() == [True, False, False, True]
    assert not c.keep(0, 32)[2, :4].any()               # no measurement: never kept
    with pytest.raises(ValueError, match="min_views"):
        c.keep(-1)
    with pytest.raises(ValueError, match="shape"):
        c.filtered(depth[:3])


def test_bad_inputs_raise_before_a_device_is_asked_for():
    from raynet_amd.consistency import check_depth_maps, check_points
    cams, _, depths, _ = ct.perturbed_plane_scene()
    pts = np.zeros((4, 3))
    for kw, match in ((dict(tol_abs=-1.0), "tol_abs"), (dict(tol_rel=float("nan")), "tol_rel"),
                      (dict(border=float("inf")), "border")):
        with pytest.raises(ValueError, match=match):
            check_points(pts, cams, depths, **kw)
        with pytest.raises(ValueError, match=match):
            check_depth_maps(depths, cams, **kw)
    with pytest.raises(ValueError, match="points"):
        check_points(np.zeros((3, 4)), cams, depths)
    with pytest.raises(ValueError, match="cameras"):
        check_depth_maps(depths)
    with pytest.raises(ValueError, match="scene"):
        check_depth_maps(depths, cams, scene=object())


def test_no_device_is_an_error_not_a_fallback(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from raynet_amd import _lib
    from raynet_amd.consistency import check_depth_maps, check_points
    cams, _, depths, _ = ct.perturbed_plane_scene()
    with pytest.raises(_lib.RaynetHipError, match="no GPU"):
        check_points(np.zeros((4, 3)), cams, depths)
    pinvs, centres = zip(*[ct.pinv_and_centre(c) for c in cams])
    with pytest.raises(_lib.RaynetHipError, match="no GPU"):
        check_depth_maps(depths, cams, P_pinvs=pinvs, centers=centres)
