"""Depth-map fusion, the host side (no GPU): the entry in the header and the ctypes table, the
argument checks and index arithmetic of the launcher (raynet_amd/csrc/raynet_fusion_args.h) as a
stand-alone program under the address and undefined-behaviour sanitizers -- nothing sanitised is
loaded into this interpreter -- TSDFVolume's file, SurfaceMesh.without_nonfinite against the
truth's cleaning, and the flags of the fuse_depth_maps script."""
import ctypes
import os
import re

import numpy as np
import pytest

import fusion_truth as ft
import abi_header
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_launcher_checks_under_sanitizers(tmp_path):
    run_host_program("fusion", tmp_path)


def test_the_launcher_and_the_kernel_use_these_checks():
    """raynet_fusion.inl decides on the header's verdict, finds its voxel and addresses the maps
    with its functions; the file is plain HIP without LDS, atomics or a square root."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_fusion.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "atomic" not in code
    assert "sqrt" not in code and "__syncthreads" not in code
    assert code.count("for (") == 1                     # the view loop is the only loop
    assert code.count("rn_fusion::integrate_args(") == 1
    assert "if (verdict == rn_fusion::INVALID)" in code
    for use in ("rn_fusion::voxel_in(", "rn_fusion::voxel_of(", "rn_fusion::axis_x(",
                "rn_fusion::axis_y(", "rn_fusion::axis_z(", "rn_fusion::map_index(",
                "rn_fusion::pixel_in(", "rn_fusion::voxels(", "rn_fusion::blocks("):
        assert use in code, use
    assert code.count("rn_view::project(") == 1         # the projection is the shared header's
    assert "h2" not in code and "cam[" not in code
    # every load of a map goes through the one guarded pixel index
    assert len(re.findall(r"a\.(depths|weights)\[", code)) == 2
    assert len(re.findall(r"a\.(depths|weights)\[pixel\]", code)) == 2
    for f in ("raynet_fusion.inl", "raynet_fusion_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
    header = open(os.path.join(CSRC, "raynet_fusion_args.h")).read()
    assert "hip" not in re.sub(r"//.*", "", header).lower()
    assert '#include "raynet_fusion.inl"' in open(os.path.join(CSRC, "raynet_hip.hip")).read()
    for f in ("raynet_fusion.inl", "raynet_fusion_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_entry_is_declared_and_bound_with_matching_types():
    """(The types of every entry, this one included: tests/test_abi.py.)"""
    from raynet_amd import _lib
    assert abi_header.prototype("rn_tsdf_integrate") == ("int", [
        "rn_ctx *ctx", "int32_t V", "const double *cameras", "int32_t H", "int32_t W",
        "const float *depths", "const float *weights", "double trunc", "double border",
        "float *tsdf", "float *weight", "void *stream"])
    assert hasattr(ctypes.CDLL(_lib.build()), "rn_tsdf_integrate")


# ------------------------------------------------------------------------------ the volume
def _volume():
    from raynet_amd.fusion import TSDFVolume
    rng = np.random.default_rng(1)
    tsdf = rng.uniform(-1, 1, (3, 4, 5)).astype(F)
    weight = rng.integers(0, 4, (3, 4, 5)).astype(F)
    tsdf[weight == 0] = 1
    return TSDFVolume(tsdf, weight, [0, 0, 0, 3, 4, 5], (3, 4, 5), 0.75)


def test_volume_file_round_trip(tmp_path):
    from raynet_amd.fusion import TSDFVolume
    v = _volume()
    path = str(tmp_path / "tsdf.npz")
    v.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["bbox", "grid_shape", "trunc", "tsdf", "weight"]
        assert z["tsdf"].dtype == F and z["weight"].dtype == F and z["tsdf"].shape == (3, 4, 5)
        assert z["grid_shape"].dtype == np.int32 and z["trunc"].dtype == np.float64
    again = TSDFVolume.load(path)
    assert again.grid_shape == (3, 4, 5) and again.trunc == 0.75
    assert np.array_equal(again.bbox, v.bbox) and again.bbox.dtype == F
    assert np.array_equal(again.tsdf.numpy().view(np.int32), v.tsdf.numpy().view(np.int32))
    assert np.array_equal(again.weight.numpy(), v.weight.numpy())
    other = str(tmp_path / "other.npz")
    np.savez(open(other, "wb"), belief=np.zeros((3, 4, 5), F), bbox=v.bbox,
             grid_shape=np.array([3, 4, 5], np.int32))
    with pytest.raises(ValueError, match="expected the arrays"):
        TSDFVolume.load(other)


def test_volume_refuses_what_is_no_volume():
    from raynet_amd.fusion import TSDFVolume
    t = np.zeros((3, 4, 5), F)
    for args, match in [((t, t, [0] * 6, (3, 4), 1.0), "grid_shape"),
                        ((t, t, [0] * 5, (3, 4, 5), 1.0), "bbox"),
                        ((t, t[:2], [0] * 6, (3, 4, 5), 1.0), "weight"),
                        ((t[:2], t, [0] * 6, (3, 4, 5), 1.0), "tsdf"),
                        ((t, t, [0] * 6, (3, 4, 5), 0.0), "trunc"),
                        ((t, t, [0] * 6, (3, 4, 5), float("nan")), "trunc")]:
        with pytest.raises(ValueError, match=match):
            TSDFVolume(*args)


def test_the_field_is_the_truths():
    v = _volume()
    for min_weight in (0.0, 2.0, 3.5):
        got = v.field(min_weight).numpy()
        want = ft.field(v.tsdf.numpy(), v.weight.numpy(), min_weight)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got.view(np.int32)[~np.isnan(got)], want.view(np.int32)[~np.isnan(want)])
    assert np.isnan(v.field(3.5).numpy()).all()
    with pytest.raises(ValueError, match="min_weight"):
        v.mesh(-1.0)
    with pytest.raises(ValueError, match="min_weight"):
        v.mesh(float("nan"))


def test_cleaning_is_the_truths_and_keeps_attributes():
    from raynet_amd.volume import SurfaceMesh
    s = ft.sphere_scene(H=30, W=40, grid=(9, 8, 7))
    tsdf, weight = ft.integrate(s["axes"], s["rows"], s["depths"], None, s["trunc"], 0.0)
    raw_v, raw_f = ft.mesh(tsdf, weight, s["axes"], s["bbox"], cleaned=False)
    want_v, want_f = ft.clean(raw_v, raw_f)
    assert not np.isfinite(raw_v).all() and 0 < len(want_f) < len(raw_f)
    rng = np.random.default_rng(0)
    normals = rng.normal(size=raw_v.shape).astype(F)
    colors = rng.integers(0, 256, size=raw_v.shape).astype(np.uint8)
    raw = SurfaceMesh(raw_v, raw_f, normals, colors)
    got = raw.without_nonfinite()
    assert got is not raw and len(raw.vertices) == len(raw_v) and len(raw.faces) == len(raw_f)
    assert got.vertices.dtype == F and got.faces.dtype == np.int32
    assert np.array_equal(got.vertices.view(np.int32), want_v.view(np.int32))
    assert np.array_equal(got.faces, want_f)
    used = np.zeros(len(raw_v), bool)
    used[raw_f[np.isfinite(raw_v)[raw_f].all((1, 2))].ravel()] = True
    assert np.array_equal(got.normals, normals[used]) and np.array_equal(got.colors, colors[used])
    # a mesh that is clean stays what it is; an empty one stays empty
    again = got.without_nonfinite()
    assert np.array_equal(again.vertices, got.vertices) and np.array_equal(again.faces, got.faces)
    none = SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)).without_nonfinite()
    assert none.empty and none.vertices.shape == (0, 3)
    # only unusable vertices: nothing is left
    nothing = SurfaceMesh(np.full((3, 3), np.nan, F), np.array([[0, 1, 2]])).without_nonfinite()
    assert nothing.empty and len(nothing.vertices) == 0


def test_fusing_needs_matching_inputs():
    from raynet_amd.fusion import fuse_depth_maps
    cams = ft.sphere_scene(H=4, W=5, grid=(3, 3, 3), V=2)["cameras"]
    maps = [np.ones((4, 5), F)] * 2
    with pytest.raises(ValueError, match="2 cameras, 1 depth maps"):
        fuse_depth_maps(maps[:1], cams, [0, 0, 0, 1, 1, 1], (3, 3, 3))
    with pytest.raises(ValueError, match="1 weight maps"):
        fuse_depth_maps(maps, cams, [0, 0, 0, 1, 1, 1], (3, 3, 3), weights=maps[:1])
    with pytest.raises(ValueError, match="no depth map"):
        fuse_depth_maps([], [], [0, 0, 0, 1, 1, 1], (3, 3, 3))


# ------------------------------------------------------------------------------ the script
def test_fuse_depth_maps_knows_its_flags(tmp_path, capsys):
    from raynet_amd.scripts import fuse_depth_maps
    p = fuse_depth_maps.build_parser()
    a = p.parse_args(["scene", "predictions", "out.ply"])
    assert (a.truncation, a.min_weight, a.border, a.pred_suffix) == (None, 0.0, 0.0, "depth")
    assert not (a.gt or a.confidence_weights or a.normals or a.color) and a.volume is None
    assert a.dataset_type == "restrepo" and a.skip_every == 0 and a.scene_idx == 1
    a = p.parse_args(["s", "p", "o.ply", "--grid_shape", "18,22,14", "--truncation", "0.3",
                      "--min_weight", "2", "--border", "1.5", "--confidence_weights",
                      "--min_confidence", "0.2", "--volume", "v.npz", "--normals", "--color",
                      "--mesh_cloud", "c.ply", "--mesh_samples", "100", "--seed", "3", "--gt",
                      "--dataset_type", "dtu", "--scene_idx", "9", "--start_end", "0,3",
                      "--skip_every", "1", "--select_neighbors_based_on", "distance",
                      "--illumination_condition", "3"])
    assert a.grid_shape == (18, 22, 14) and a.truncation == 0.3 and a.min_weight == 2.0
    assert a.start_end == (0, 3) and a.mesh_samples == 100 and a.volume == "v.npz" and a.gt
    out = str(tmp_path / "out.ply")
    for argv, message in [
            (["--truncation", "0"], "--truncation"), (["--truncation", "nan"], "--truncation"),
            (["--truncation", "inf"], "--truncation"), (["--border", "-1"], "--border"),
            (["--border", "nan"], "--border"), (["--min_weight", "-1"], "--min_weight"),
            (["--grid_shape", "4,4"], "--grid_shape"), (["--grid_shape", "4,0,4"], "--grid_shape"),
            (["--start_end", "3"], "--start_end"), (["--mesh_cloud", "c.ply"], "--mesh_samples"),
            (["--mesh_samples", "5"], "--mesh_cloud"),
            (["--min_confidence", "0.5"], "--confidence_weights"),
            (["--gt", "--confidence_weights"], "no confidence")]:
        with pytest.raises(SystemExit) as e:
            fuse_depth_maps.main(["scene", "predictions", out] + argv)
        assert e.value.code == 2
        assert message in capsys.readouterr().err, argv
    assert not os.path.exists(out)
