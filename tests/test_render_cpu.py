"""Rendering a mesh, the host side (no GPU): the argument checks and the lane mappings of
raynet_amd/csrc/raynet_render_args.h as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter --, the entry
in the header, in the ctypes table and in the built library, metrics.photometric_error on
hand-made arrays, MeshRender's images on hand-made planes, and what the command line refuses."""
import ctypes
import os
import re

import numpy as np
import pytest

import render_truth as rd
import abi_header
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_every_verdict_and_both_lane_mappings_under_sanitizers(tmp_path):
    run_host_program("render", tmp_path)


def test_the_entry_is_declared_bound_and_built_with_matching_types():
    """(The types of every entry, this one included, in the table and on the loaded function:
    tests/test_abi.py.)"""
    from raynet_amd import _lib
    arguments = ["rn_ctx *ctx", "const float *nodes", "const float *leaves", "int64_t nv",
                 "const float *vertices", "int64_t nf", "const int32_t *faces", "const float *colors",
                 "int32_t C", "const float *normals", "int32_t V", "const float *cameras",
                 "int32_t H", "int32_t W", "int32_t *face", "float *depth", "float *bary",
                 "float *color", "float *normal", "void *stream"]
    assert abi_header.prototype("rn_mesh_render") == ("int", arguments)
    assert hasattr(ctypes.CDLL(_lib.build()), "rn_mesh_render")
    lib = _lib.load()
    # without a context the entry refuses before it touches anything: no GPU needed
    null = ctypes.c_void_p(0)
    assert lib.rn_mesh_render(null, null, null, 3, null, 1, null, null, 0, null, 1, null, 4, 4,
                              null, null, null, null, null, null) == -1
    # the unit includes the kernel behind the traversal it uses, and the build knows both files
    unit = open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert unit.count('#include "raynet_render.inl"') == 1
    assert unit.index('"raynet_mesh.inl"') < unit.index('"raynet_render.inl"')
    for f in ("raynet_render.inl", "raynet_render_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_kernel_uses_the_header_and_leaves_the_traversal_alone():
    src = open(os.path.join(CSRC, "raynet_render.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert code.count("rn_render::render_args(") == 1 and code.count("mesh_first_hit(") == 1
    assert "if (verdict == rn_render::INVALID)" in code
    assert "if (verdict == rn_render::EMPTY) return RN_OK;" in code
    assert "mesh_test_leaf" not in code and "asm" not in code and "atomic" not in code
    assert "__shared__ uint32_t stack[MESH_STACK * MESH_RAY_BLOCK];" in code
    for use in ("rn_render::pixel_of_tile(", "rn_render::pixel_of_row(", "rn_render::pixel_index(",
                "rn_render::face_in(", "rn_render::vertex_in(", "rn_render::blocks("):
        assert use in code, use
    header = open(os.path.join(CSRC, "raynet_render_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "#pragma once" in header
    assert '#include "raynet_mesh_args.h"' in header and "sizes_ok(nv, nf)" in header
    mesh = open(os.path.join(CSRC, "raynet_mesh.inl")).read()
    assert "render" not in mesh.lower()


# ------------------------------------------------------------------------------ the score
def test_photometric_error_on_hand_made_arrays():
    from raynet_amd.metrics import photometric_error
    image = np.zeros((4, 5, 3), F)
    image[..., 1] = 0.5
    mask = np.zeros((4, 5), bool)
    mask[1:3, 1:4] = True                           # 6 of 20 pixels
    same = photometric_error(image, image.copy(), mask)
    assert same == dict(coverage=0.3, mae=0.0, mse=0.0, psnr=float("inf"))
    none = photometric_error(image, image + 1, np.zeros((4, 5), bool))
    assert none["coverage"] == 0.0
    assert all(np.isnan(none[k]) for k in ("mae", "mse", "psnr"))
    # off by 0.1 in one channel of three: mae 0.1 / 3, mse 0.01 / 3; outside the mask: anything
    other = image.copy()
    other[..., 0] += 0.1
    other[~mask] = 7.0
    got = photometric_error(other, image, mask)
    assert got["coverage"] == 0.3
    assert got["mae"] == pytest.approx(0.1 / 3, rel=1e-6) and got["mse"] == pytest.approx(0.01 / 3, rel=1e-6)
    assert got["psnr"] == pytest.approx(10 * np.log10(300.0), rel=1e-6)
    assert all(isinstance(v, float) for v in got.values())
    # a grey pair, everything covered
    grey = photometric_error(np.full((2, 2), 0.25), np.full((2, 2), 0.75), np.ones((2, 2), bool))
    assert grey == dict(coverage=1.0, mae=0.5, mse=0.25, psnr=pytest.approx(10 * np.log10(4.0)))
    for bad in ((image, image[:3], mask), (image, image, mask[:3]), (image[0, 0], image[0, 0], mask)):
        with pytest.raises(ValueError, match="rendered"):
            photometric_error(*bad)


def test_the_images_of_a_render_from_hand_made_planes():
    import torch
    from raynet_amd.render import MeshRender, camera_rows
    from raynet_amd.synthetic import ring_cameras
    face = torch.tensor([[[0, -1], [2, 5]]], dtype=torch.int32)
    color = torch.tensor([[[[1.0, 0.5, 0.0], [0.3, 0.3, 0.3]], [[2.0, -1.0, 0.25], [0.0, 0.0, 1.0]]]])
    normal = torch.tensor([[[[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], [[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]]])
    r = MeshRender(face, torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, 2), color, normal)
    assert r.mask.tolist() == [[[True, False], [True, True]]]
    rgb = r.rgb8(0, background=(9, 8, 7))
    assert rgb.dtype == np.uint8 and rgb.tolist() == [[[255, 128, 0], [9, 8, 7]],
                                                      [[255, 0, 64], [0, 0, 255]]]
    assert r.normal_rgb8(0).tolist() == [[[128, 128, 255], [0, 0, 0]], [[0, 128, 128], [128, 255, 128]]]
    grey = MeshRender(face, r.depth, r.bary, color[..., :1].contiguous(), None)
    assert grey.rgb8(0).tolist() == [[[255] * 3, [0] * 3], [[255] * 3, [0] * 3]]
    for call in (grey.normal_rgb8, lambda v: grey.shaded8(v, [])):
        with pytest.raises(ValueError, match="without normals"):
            call(0)
    with pytest.raises(ValueError, match="without colours"):
        MeshRender(face, r.depth, r.bary, None, normal).rgb8(0)
    # the headlight: a normal that looks back along the pixel's ray is white, one that looks away black
    cams = ring_cameras(1, 2, 2)
    rows = camera_rows(cams)
    assert rows.shape == (1, 15) and rows.dtype == F and np.array_equal(rows, rd.camera_rows(cams))
    assert camera_rows([]).shape == (0, 15)
    o, dst = rd.view_rays(rows[0], 2, 2)
    back = o - dst
    back /= np.linalg.norm(back, axis=1)[:, None]
    lit = MeshRender(torch.zeros(1, 2, 2, dtype=torch.int32), r.depth, r.bary, None,
                     torch.from_numpy(back.reshape(1, 2, 2, 3).astype(F)))
    assert (lit.shaded8(0, cams) == 255).all()
    lit.normal = -lit.normal
    assert (lit.shaded8(0, cams) == 0).all()


# ------------------------------------------------------------------------------ the command line
def test_what_the_command_line_refuses(tmp_path, capsys):
    from raynet_amd.scripts import render_mesh, render_volume
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = rd.icosphere(0)
    plain, coloured = str(tmp_path / "plain.ply"), str(tmp_path / "coloured.ply")
    SurfaceMesh(vertices, faces).save_ply(plain)
    SurfaceMesh(vertices, faces, colors=np.full((len(vertices), 3), 200, np.uint8)).save_ply(coloured)
    empty = str(tmp_path / "empty.ply")
    SurfaceMesh(vertices, np.zeros((0, 3), np.int32), colors=np.zeros((12, 3), np.uint8)).save_ply(empty)
    out = str(tmp_path / "out")
    cases = [([plain, out, "--planes", "color"], "--planes color"),
             ([plain, out, "--compare"], "--compare"),
             ([coloured, out, "--planes", "depth", "--compare"], "--compare"),
             ([coloured, out, "--planes", "colour"], "--planes"),
             ([coloured, out, "--planes", ","], "--planes"),
             ([coloured, out, "--background", "0,0"], "--background"),
             ([coloured, out, "--background", "0,0,256"], "--background"),
             ([coloured, out, "--background", "red"], "--background"),
             ([coloured, out, "--start_end", "0"], "--start_end"),
             ([coloured, out, "--dataset_type", "kitti"], "--dataset_type"),
             ([empty, out], "empty"),
             ([str(tmp_path / "missing.ply"), out], "no such file")]
    for argv, named in cases:
        with pytest.raises(SystemExit) as e:
            render_mesh.main(["scene"] + argv)
        assert e.value.code == 2, argv
        assert named in capsys.readouterr().err, argv
    assert not os.path.exists(out)
    # the dataset flags are render_volume's
    mine = {a.dest: (a.default, a.choices) for a in render_mesh.build_parser()._actions}
    for a in render_volume.build_parser()._actions:
        if a.dest in ("dataset_type", "scene_idx", "start_end", "skip_every",
                      "select_neighbors_based_on", "illumination_condition"):
            assert mine[a.dest] == (a.default, a.choices), a.dest
    assert render_mesh.PLANES == ("color", "normals", "shaded", "depth", "faces")
    for text in (open(os.path.join(REPO, "README.md")).read(),
                 open(os.path.join(REPO, "tools", "README.md")).read()):
        assert "render_mesh" in text or "render_bench" in text
    assert "raynet_amd.scripts.render_mesh" in open(os.path.join(REPO, "README.md")).read()


def test_without_a_gpu_there_is_no_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from raynet_amd import _lib
    from raynet_amd.synthetic import ring_cameras
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = rd.icosphere(0)
    with pytest.raises(_lib.RaynetHipError):
        SurfaceMesh(vertices, faces).render(ring_cameras(1, 4, 4), 4, 4)
    with pytest.raises(ValueError, match="empty"):
        SurfaceMesh(vertices, np.zeros((0, 3), np.int32)).render(ring_cameras(1, 4, 4), 4, 4)
