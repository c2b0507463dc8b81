"""Normals and colours, the host side (no GPU): the two entries in the header and the ctypes table,
SurfaceMesh's and Pointcloud's files, the new flags of render_volume and convert_to_pointcloud,
and the argument checks and index arithmetic of the launchers
(raynet_amd/csrc/raynet_appearance_args.h) as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import appearance_truth as at
import isosurface_truth as it
from conftest import REPO
from host_program import run_host_program

F = np.float32


@pytest.mark.parametrize("name,params", [
    ("rn_vertex_area_normals",
     ["rn_ctx *ctx", "int64_t nv", "const float *vertices", "int64_t nf", "const int32_t *faces",
      "const int32_t *offsets", "const int32_t *corners", "float *normals", "void *stream"]),
    ("rn_project_colors",
     ["rn_ctx *ctx", "int64_t n", "const float *points", "const float *normals", "int32_t V",
      "const double *cameras", "int32_t H", "int32_t W", "int32_t C", "const float *images",
      "const float *depths", "double tol", "double min_cos", "double border", "int32_t mode",
      "float *colors", "float *weight", "uint32_t *views", "void *stream"]),
])
def test_entries_are_declared_and_bound_with_matching_types(name, params):
    """(The types of every entry, these two included: tests/test_abi.py.)"""
    from raynet_amd import _lib
    assert abi_header.prototype(name) == ("int", params)
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(params)
    assert hasattr(ctypes.CDLL(_lib.build()), name)


def test_the_kernel_file_is_plain_hip_and_listed():
    from raynet_amd import _lib
    csrc = os.path.join(REPO, "raynet_amd", "csrc")
    src = open(os.path.join(csrc, "raynet_appearance.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "atomic" not in code
    assert "sqrt" not in code
    for f in ("raynet_appearance.inl", "raynet_appearance_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(csrc, f)).read(),
                             re.M), f
    assert '#include "raynet_appearance.inl"' in open(os.path.join(csrc, "raynet_hip.hip")).read()
    # the launchers decide on the header's verdicts, the kernels read through its guards
    assert "rn_app::normals_args(" in src and "rn_app::colors_args(" in src
    for guard in ("rn_app::vertex_in(", "rn_app::corner_in(", "rn_app::clamp_slot(",
                  "rn_app::pixel_in(", "rn_app::image_index(", "rn_app::depth_index("):
        assert guard in src, guard
    # the names are the shared header's (tests/test_views_cpu.py), under which the bake calls the
    # per-view step; this kernel keeps it written out (DESIGN.md section 20 says why)
    assert "rn_view::observe<" not in code and code.count("X = h0 / h2, Y = h1 / h2;") == 1
    header = open(os.path.join(csrc, "raynet_appearance_args.h")).read()
    assert "using rn_view::CAMERA_DOUBLES, rn_view::image_index, rn_view::pixel_in;" in header
    assert "return rn_view::map_index(v, y, x, H, W);" in header        # rn_app::depth_index
    # one instance per channel count
    for c in "1234":
        assert "k_project_colors<%s>" % c in src
    for f in ("raynet_appearance.inl", "raynet_appearance_args.h", "raynet_views_args.h"):
        assert os.path.join(csrc, f) in _lib.sources(), f


def test_launcher_checks_under_sanitizers(tmp_path):
    run_host_program("appearance", tmp_path)


# ------------------------------------------------------------------------- SurfaceMesh's file
def _ball():
    belief = it.logistic_ball()
    bbox, axes = it.unit_frame(belief.shape)
    return it.extract(belief, 0.5, True, axes, bbox)


def _plain_writer(path, vertices, faces):
    """The file SurfaceMesh.save_ply wrote before meshes had attributes, byte for byte."""
    rows = np.empty((len(faces),), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rows["n"] = 3
    rows["v"] = faces
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\ncomment raynet_amd surface mesh\n"
                 "element vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(vertices), len(faces))).encode())
        vertices.astype("<f4").tofile(f)
        rows.tofile(f)


def test_a_mesh_without_attributes_writes_the_file_it_always_wrote(tmp_path):
    from raynet_amd.volume import SurfaceMesh
    v, f = _ball()
    mesh = SurfaceMesh(v, f)
    assert mesh.normals is None and mesh.colors is None
    mesh.save_ply(str(tmp_path / "now.ply"))
    _plain_writer(str(tmp_path / "then.ply"), v, f)
    assert open(str(tmp_path / "now.ply"), "rb").read() == open(str(tmp_path / "then.ply"), "rb").read()
    again = SurfaceMesh.load_ply(str(tmp_path / "now.ply"))
    assert again.normals is None and again.colors is None


@pytest.mark.parametrize("with_normals,with_colors", [(True, True), (True, False), (False, True)])
def test_ply_round_trip_with_normals_and_colours(tmp_path, with_normals, with_colors):
    from raynet_amd.appearance import normalized
    from raynet_amd.common.mesh_io import parse_gt_data_from_ply
    from raynet_amd.volume import SurfaceMesh
    v, f = _ball()
    rng = np.random.default_rng(5)
    normals = normalized(at.area_normals(v, f)) if with_normals else None
    colors = rng.integers(0, 256, size=v.shape).astype(np.uint8) if with_colors else None
    mesh = SurfaceMesh(v, f, normals, colors)
    path = str(tmp_path / "ball.ply")
    mesh.save_ply(path)
    head = open(path, "rb").read(600).split(b"end_header\n")[0].decode().split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    want = ["element vertex 756", "property float x", "property float y", "property float z"]
    if with_normals:
        want += ["property float nx", "property float ny", "property float nz"]
    if with_colors:
        want += ["property uchar red", "property uchar green", "property uchar blue"]
    want += ["element face 1508", "property list uchar int vertex_indices"]
    assert [l for l in head if l.startswith(("element", "property"))] == want
    # the coloured file loads through the ground-truth reader: the attributes are its `normals`
    points, rest, faces = parse_gt_data_from_ply(path)
    assert np.array_equal(points.view(np.int32), v.view(np.int32)) and np.array_equal(faces, f)
    assert rest.shape == (756, 3 * with_normals + 3 * with_colors)
    again = SurfaceMesh.load_ply(path)
    assert np.array_equal(again.vertices.view(np.int32), v.view(np.int32))
    assert np.array_equal(again.faces, f) and again.faces.dtype == np.int32
    if with_normals:
        assert again.normals.dtype == F
        assert np.array_equal(again.normals.view(np.int32), normals.view(np.int32))
        length = np.sqrt((again.normals.astype(np.float64) ** 2).sum(1))
        assert np.abs(length - 1).max() < 1e-6
    else:
        assert again.normals is None
    if with_colors:
        assert again.colors.dtype == np.uint8 and np.array_equal(again.colors, colors)
    else:
        assert again.colors is None
    with pytest.raises(ValueError, match="normals"):
        SurfaceMesh(v, f, normals=np.zeros((3, 3), F))
    with pytest.raises(ValueError, match="colors"):
        SurfaceMesh(v, f, colors=np.zeros((len(v), 4), np.uint8))


def test_unit_normals_keep_zero_vectors_and_colours_round_to_bytes():
    from raynet_amd.appearance import normalized, to_rgb8
    n = normalized(np.array([[0, 0, 0], [3, 0, 4], [0, -2, 0], [1e-30, 0, 0]], F))
    assert np.array_equal(n[0], [0, 0, 0]) and np.allclose(n[1], [0.6, 0, 0.8])
    assert np.array_equal(n[2], [0, -1, 0]) and np.array_equal(n[3], [1, 0, 0])
    assert not np.isnan(n).any()
    c = np.array([[0.0, 0.5, 1.0], [-0.2, 1.7, 0.25], [0.1, 0.2, 0.3]], F)
    rgb = to_rgb8(c, np.array([True, True, False]), unseen=(0.5, 0.5, 0.5))
    assert rgb.dtype == np.uint8
    assert rgb.tolist() == [[0, 128, 255], [0, 255, 64], [128, 128, 128]]      # rint: half to even
    assert to_rgb8(np.array([[0.2]], F)).tolist() == [[51, 51, 51]]             # grey
    assert to_rgb8(np.array([[0.2, 0.4, 0.6, 0.9]], F)).tolist() == [[51, 102, 153]]


def test_more_than_32_views_is_refused_with_advice():
    from raynet_amd.appearance import project_colors
    cams, images, depths = at.plane_scene()
    with pytest.raises(ValueError, match="choose the\\s+frames"):
        project_colors(np.zeros((4, 3), F), cams * 11, list(images) * 11)
    with pytest.raises(ValueError, match="mode"):
        project_colors(np.zeros((4, 3), F), cams, list(images), mode="median")
    with pytest.raises(ValueError, match="2 images"):
        project_colors(np.zeros((4, 3), F), cams, list(images)[:2])


def test_camera_rows_are_the_truths():
    from raynet_amd.appearance import pack_cameras
    from raynet_amd.common.camera import Camera
    cams = [Camera.look_at([2.0, 0.5 * k, 1.0], [0, 0, 0], 30.0, 24, 32) for k in range(3)]
    rows = pack_cameras(cams)
    assert rows.dtype == np.float64 and rows.shape == (3, 15)
    assert np.array_equal(rows, at.pack_cameras(cams))
    assert np.array_equal(rows[1, :12].reshape(3, 4), cams[1].P)
    assert np.array_equal(rows[1, 12:], cams[1].center.ravel()[:3].astype(np.float64))


def test_pointcloud_rgb_file(tmp_path):
    from raynet_amd.common.mesh_io import read_ply
    from raynet_amd.pointcloud import Pointcloud
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(3, 50)).astype(F)
    colors = rng.integers(0, 256, size=(50, 3)).astype(np.uint8)
    cloud = Pointcloud(pts)
    path = str(tmp_path / "rgb.ply")
    cloud.save_rgb_ply(path, colors)
    # the header layout of save_colored_ply
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    assert [l for l in head if l.startswith(("element", "property"))] == [
        "element vertex 50", "property float x", "property float y", "property float z",
        "property uchar red", "property uchar green", "property uchar blue"]
    v = read_ply(path)["vertex"]
    assert np.array_equal(np.stack([v[k] for k in "xyz"]), pts)
    assert np.array_equal(np.stack([v[k] for k in ("red", "green", "blue")], 1), colors)
    with pytest.raises(ValueError, match="colors"):
        cloud.save_rgb_ply(path, colors[:10])
    with pytest.raises(ValueError, match="colors"):
        cloud.save_rgb_ply(path, colors.astype(F))


# ------------------------------------------------------------------------------ the scripts
def test_render_volume_knows_the_colour_flags(tmp_path, capsys):
    from raynet_amd.scripts import render_volume
    p = render_volume.build_parser()
    a = p.parse_args(["scene", "occupancy.npz", "out"])
    assert (a.color, a.color_mode, a.depth_tolerance) == (False, "blend", 1.0)
    assert a.mesh is None and a.plane == "depth" and a.threshold == 0.5        # as they were
    a = p.parse_args(["s", "o.npz", "out", "--mesh", "m.ply", "--color", "--color_mode", "best",
                      "--depth_tolerance", "2.5"])
    assert (a.mesh, a.color, a.color_mode, a.depth_tolerance) == ("m.ply", True, "best", 2.5)
    occupancy = str(tmp_path / "occupancy.npz")
    open(occupancy, "wb").close()
    for argv, message in [
            (["--color"], "--color goes with --mesh"),
            (["--mesh", "m.ply", "--color", "--depth_tolerance", "-1"], "--depth_tolerance"),
            (["--mesh", "m.ply", "--color", "--depth_tolerance", "inf"], "--depth_tolerance"),
            (["--mesh", "m.ply", "--color", "--depth_tolerance", "nan"], "--depth_tolerance"),
            (["--mesh", "m.ply", "--color", "--color_mode", "median"], "--color_mode")]:
        with pytest.raises(SystemExit) as e:
            render_volume.main(["scene", occupancy, str(tmp_path / "out")] + argv)
        assert e.value.code == 2
        assert message in capsys.readouterr().err
    assert not os.path.exists(str(tmp_path / "out"))


def test_convert_to_pointcloud_knows_the_colour_flag(capsys):
    from raynet_amd.scripts import convert_to_pointcloud
    p = convert_to_pointcloud.build_parser()
    a = p.parse_args(["scene", "predictions", "out"])
    assert a.color is False and a.consistency_threshold == 0.75 and a.borders == 40
    a = p.parse_args(["scene", "predictions", "out", "--color", "--consistency_threshold", "0.1"])
    assert a.color is True and a.consistency_threshold == 0.1
    with pytest.raises(SystemExit) as e:
        convert_to_pointcloud.main(["scene", "predictions", "out", "--color",
                                    "--consistency_threshold", "-0.5"])
    assert e.value.code == 2 and "--consistency_threshold" in capsys.readouterr().err
