"""The texture atlas, the host side (no GPU): the argument checks, the layout and the lane mappings
of raynet_amd/csrc/raynet_texture_args.h as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter --, the two
entries in the header, in the ctypes table and in the built library, what the new kernel file may
contain, what the three command lines refuse, and the OBJ triple of a hand-made mesh read back."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")

BAKE = ["rn_ctx *ctx", "int64_t nv", "const float *vertices", "int64_t nf", "const int32_t *faces",
        "const float *normals", "int32_t T", "int32_t cells_per_row", "int32_t V",
        "const double *cameras", "int32_t H", "int32_t W", "int32_t C", "const float *images",
        "const float *depths", "double tol", "double min_cos", "double border", "int32_t mode",
        "float *texture", "float *weight", "uint32_t *views", "void *stream"]
SAMPLE = ["rn_ctx *ctx", "int64_t n", "const int32_t *face", "const float *bary", "int64_t nf",
          "int32_t T", "int32_t cells_per_row", "int32_t C", "const float *texture",
          "int32_t bilinear", "float *color", "void *stream"]


def test_every_verdict_the_layout_and_both_lane_mappings_under_sanitizers(tmp_path):
    run_host_program("texture", tmp_path)


@pytest.mark.parametrize("name,arguments", [("rn_texture_bake", BAKE), ("rn_texture_sample", SAMPLE)])
def test_the_entries_are_declared_bound_and_built_with_matching_types(name, arguments):
    """(The types of every entry, these two included, in the table and on the loaded function:
    tests/test_abi.py.)"""
    from raynet_amd import _lib
    assert abi_header.prototype(name) == ("int", arguments)
    assert hasattr(ctypes.CDLL(_lib.build()), name)
    fn = getattr(_lib.load(), name)
    # without a context the entry refuses before it touches anything: no GPU needed
    null = ctypes.c_void_p(0)
    values = [null if "*" in a else (0.0 if a.startswith("double") else 1) for a in arguments]
    assert fn(*values) == -1
    unit = open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert unit.count('#include "raynet_texture.inl"') == 1
    for f in ("raynet_texture.inl", "raynet_texture_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_kernels_are_plain_and_use_the_header():
    src = open(os.path.join(CSRC, "raynet_texture.inl")).read()
    for word in ("asm", "__shared__", "atomic", "sqrt"):
        assert word not in src, word
    code = re.sub(r"//.*", "", src)
    assert code.count("rn_tex::bake_args(") == 1 and code.count("rn_tex::sample_args(") == 1
    assert code.count("if (verdict == rn_tex::INVALID)") == 2
    assert code.count("if (verdict == rn_tex::EMPTY) return RN_OK;") == 2
    for use in ("rn_tex::texel_of_tile(", "rn_tex::texel_of_row(", "rn_tex::owner_of(",
                "rn_tex::raw_coordinate(", "rn_tex::chart_coordinate(", "rn_tex::texel_index(",
                "rn_tex::face_in(", "rn_tex::vertex_in(", "rn_tex::layout_of(", "rn_tex::blocks("):
        assert use in code, use
    # the per-view step is the shared header's, called once; there every image and depth load goes
    # through image_index / map_index with pixel_in-guarded coordinates, and the bake itself loads
    # neither
    assert code.count("rn_view::observe<") == 1 and not re.search(r"a\.(images|depths)\[", code)
    views = re.sub(r"//.*", "", open(os.path.join(CSRC, "raynet_views_args.h")).read())
    assert len(re.findall(r"a\.images\[image_index\(", views)) == 4 == views.count("a.images[")
    assert len(re.findall(r"a\.depths\[map_index\(", views)) == 1 == views.count("a.depths[")
    for guard in ("pixel_in(yr, a.H) ? yr : 0", "pixel_in(xr, a.W) ? xr : 0",
                  "x0 = pixel_in(x0, a.W) ? x0 : 0;", "y0 = pixel_in(y0, a.H) ? y0 : 0;",
                  "std::min(x0 + 1, a.W - 1)", "std::min(y0 + 1, a.H - 1)"):
        assert views.count(guard) == 1, guard
    assert src.count("constexpr bool TEXTURE_TILED = true;") == 1
    header = open(os.path.join(CSRC, "raynet_texture_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "#pragma once" in header and "namespace rn_tex" in header
    assert '#include "raynet_mesh_args.h"' in header and "sizes_ok(nv, nf)" in header
    # the older stages do not know the new one
    for name in ("raynet_appearance.inl", "raynet_render.inl", "raynet_appearance_args.h",
                 "raynet_render_args.h", "raynet_views_args.h"):
        assert "texture" not in open(os.path.join(CSRC, name)).read().lower(), name


# ------------------------------------------------------------------------------ the command lines
def test_what_the_command_lines_refuse(tmp_path, capsys):
    import render_truth as rd
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags, render_mesh, render_volume, texture_flags
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = rd.icosphere(0)
    ply = str(tmp_path / "coloured.ply")
    SurfaceMesh(vertices, faces, colors=np.full((len(vertices), 3), 200, np.uint8)).save_ply(ply)
    out = str(tmp_path / "out")
    fuse = ["scene", "predictions", str(tmp_path / "mesh.ply")]
    volume = ["scene", "occupancy.npz", out]
    cases = [(render_mesh, ["scene", ply, out, "--texture", "0"], "--texture"),
             (render_mesh, ["scene", ply, out, "--texture", "1025"], "--texture"),
             (render_mesh, ["scene", ply, out, "--texture", "four"], "--texture"),
             (render_mesh, ["scene", ply, out, "--texture_mode", "best"], "--texture_mode"),
             (render_mesh, ["scene", ply, out, "--texture_normals", "vertex"], "--texture_normals"),
             (render_mesh, ["scene", ply, out, "--texture_nearest"], "--texture_nearest"),
             (render_mesh, ["scene", ply, out, "--texture", "4", "--texture_mode", "mean"], "--texture_mode"),
             (render_mesh, ["scene", ply, out, "--texture_tolerance", "0.1"], "--texture_tolerance"),
             (render_mesh, ["scene", ply, out, "--texture", "4", "--texture_tolerance", "-1"],
              "--texture_tolerance"),
             (fuse_depth_maps, fuse + ["--texture", "0"], "--texture"),
             (fuse_depth_maps, fuse + ["--texture", "-3"], "--texture"),
             (fuse_depth_maps, fuse + ["--texture", "2000"], "--texture"),
             (fuse_depth_maps, fuse + ["--texture_mode", "blend"], "--texture_mode"),
             (fuse_depth_maps, fuse + ["--texture_normals", "face"], "--texture_normals"),
             (fuse_depth_maps, fuse + ["--texture", "4", "--texture_normals", "smooth"], "--texture_normals"),
             (fuse_depth_maps, fuse + ["--texture_nearest"], "--texture_nearest"),
             (render_volume, volume + ["--mesh", ply, "--texture", "0"], "--texture"),
             (render_volume, volume + ["--mesh", ply, "--texture_mode", "best"], "--texture_mode"),
             (render_volume, volume + ["--texture", "4"], "--mesh")]
    for module, argv, named in cases:
        with pytest.raises(SystemExit) as e:
            module.main(argv)
        assert e.value.code == 2, argv
        assert named in capsys.readouterr().err, argv
    assert not os.path.exists(out)
    # the stages' flags are the tuple they were; the texture's are a tuple of their own
    assert texture_flags.TEXTURE_FLAGS == ("texture", "texture_mode", "texture_normals")
    assert not set(texture_flags.TEXTURE_FLAGS) & set(mesh_flags.FLAGS)
    for module in (fuse_depth_maps, render_volume, render_mesh):
        dests = {a.dest: a for a in module.build_parser()._actions}
        for name in texture_flags.TEXTURE_FLAGS:
            assert dests[name].default is None, (module.__name__, name)
        assert ("texture_nearest" in dests) == (module is render_mesh)
    assert render_mesh.PLANES == ("color", "normals", "shaded", "depth", "faces")
    for name in ("README.md", os.path.join("tools", "README.md"), "INTEGRATION.md", "DESIGN.md"):
        assert "texture" in open(os.path.join(REPO, name)).read(), name


# ------------------------------------------------------------------------------ the file
def test_the_obj_triple_of_a_two_face_mesh_reads_back(tmp_path):
    import torch
    from PIL import Image as PILImage
    from raynet_amd import texture as tx
    from raynet_amd.volume import SurfaceMesh
    vertices = np.array([[0, 0, 0], [1, 0, 0.25], [1, 1, 0], [0, 1, -0.5]], F)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    T = 3
    layout = tx.atlas_layout(2, T)
    assert (layout.Wt, layout.Ht, layout.cells_per_row) == (8, 8, 1)
    rng = np.random.default_rng(0)
    colours = rng.random((8, 8, 3)).astype(F)
    views = np.ones((8, 8), np.int32)
    views[2, 3] = views[6, 6] = 0                   # one texel of either face that no view saw
    baked = tx.MeshTexture(torch.from_numpy(colours), torch.ones((8, 8)), torch.from_numpy(views),
                           layout)
    mesh = SurfaceMesh(vertices, faces)
    paths = mesh.save_obj(str(tmp_path / "quad.ply"), baked, unseen=(1.0, 0.0, 0.5))
    assert [os.path.basename(p) for p in paths] == ["quad.obj", "quad.mtl", "quad.png"]
    assert all(os.path.isfile(p) for p in paths)
    v, vt, f, other = [], [], [], []
    for line in open(paths[0]).read().splitlines():
        word = line.split()
        if not word or word[0] == "#":
            continue
        if word[0] == "v":
            v.append([float(x) for x in word[1:]])
        elif word[0] == "vt":
            vt.append([float(x) for x in word[1:]])
        elif word[0] == "f":
            f.append([[int(k) for k in corner.split("/")] for corner in word[1:]])
        else:
            other.append(word)
    assert other == [["mtllib", "quad.mtl"], ["usemtl", "quad"]]
    assert np.array_equal(np.array(v, F), vertices)
    f = np.array(f)
    assert f.shape == (2, 3, 2) and np.array_equal(f[..., 0] - 1, faces)          # 1-based
    uvs = np.array(vt)[f[..., 1] - 1]
    assert np.array_equal(uvs, tx.face_uvs(2, layout))
    # the texture coordinates are the centres of the chart's corner texels, v upwards
    x, y = uvs[..., 0] * 8 - 0.5, (1 - uvs[..., 1]) * 8 - 0.5
    assert np.allclose(x, [[1, T + 1, 1], [T + 3, 3, T + 3]], atol=1e-12)
    assert np.allclose(y, [[1, 1, T + 1], [T + 3, T + 3, 3]], atol=1e-12)
    mtl = open(paths[1]).read().split("\n")
    assert mtl[0] == "newmtl quad" and "map_Kd quad.png" in mtl
    png = np.asarray(PILImage.open(paths[2]))
    want = np.rint(np.clip(colours, 0, 1) * 255).astype(np.uint8)
    want[2, 3] = want[6, 6] = (255, 0, 128)
    assert png.shape == (8, 8, 3) and np.array_equal(png, want)                    # row 0 on top
    assert np.array_equal(baked.rgb8(unseen=(1.0, 0.0, 0.5)), want)
    # an empty texel keeps what it has: of one face's atlas the upper half is nobody's
    lone = tx.MeshTexture(torch.zeros((8, 8, 3)), torch.zeros((8, 8)),
                          torch.zeros((8, 8), dtype=torch.int32), tx.atlas_layout(1, T))
    filled = lone.filled(unseen=(0.25, 0.25, 0.25))
    assert (filled[0, 0] == 0.25).all() and (filled[7, 7] == 0).all()
    assert (filled[..., 0] == 0.25).sum() == (T + 4) * (T + 5) // 2
    with pytest.raises(ValueError, match="faces"):
        mesh.save_obj(str(tmp_path / "other.obj"), lone)


def test_without_a_gpu_there_is_no_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import render_truth as rd
    from raynet_amd import _lib, texture as tx
    from raynet_amd.render import MeshRender
    from raynet_amd.synthetic import ring_cameras
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = rd.icosphere(0)
    mesh = SurfaceMesh(vertices, faces)
    cams = ring_cameras(2, 4, 4)
    images = [np.zeros((4, 4, 3), F)] * 2
    with pytest.raises(_lib.RaynetHipError):
        tx.bake_texture(mesh, cams, images, 4)
    with pytest.raises(ValueError, match="empty"):
        tx.bake_texture(SurfaceMesh(vertices, np.zeros((0, 3), np.int32)), cams, images, 4)
    for bad in (dict(mode="mean"), dict(normals="smooth")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            tx.bake_texture(mesh, cams, images, 4, **bad)
    with pytest.raises(ValueError, match="32"):
        tx.bake_texture(mesh, ring_cameras(33, 4, 4), images * 17, 4)
    layout = tx.atlas_layout(len(faces), 2)
    baked = tx.MeshTexture(torch.zeros((layout.Ht, layout.Wt, 3)), None, None, layout)
    render = MeshRender(torch.zeros((1, 2, 2), dtype=torch.int32), None, torch.zeros((1, 2, 2, 2)),
                        None, None)
    with pytest.raises(_lib.RaynetHipError):
        render.textured(baked)
