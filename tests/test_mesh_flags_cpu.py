"""The mesh-cleanup flags of fuse_depth_maps and render_volume (raynet_amd/scripts/mesh_flags.py,
no GPU): every usage error of the ten flags in both scripts, message and exit code against the
literal texts the three per-stage modules had before they became one; the chain of the stages and
the voxel arithmetic of `apply`; and the one statement of the mesh guards in the csrc headers."""
import os
import re
import types

import numpy as np
import pytest

from conftest import REPO

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")

# argv -> the message of parser.error, in both scripts (render_volume with --mesh PATH)
USAGE_ERRORS = [
    (["--min_component_faces", "0"], "--min_component_faces takes a number of faces, 1 or more"),
    (["--min_component_faces", "-3"], "--min_component_faces takes a number of faces, 1 or more"),
    (["--keep_largest", "0"], "--keep_largest takes a number of components, 1 or more"),
    (["--min_component_fraction", "0"], "--min_component_fraction takes a fraction in (0, 1]"),
    (["--min_component_fraction", "1.5"], "--min_component_fraction takes a fraction in (0, 1]"),
    (["--min_component_fraction", "nan"], "--min_component_fraction takes a fraction in (0, 1]"),
    (["--simplify", "0"], "--simplify takes a positive, finite number of voxel sides"),
    (["--simplify", "-2"], "--simplify takes a positive, finite number of voxel sides"),
    (["--simplify", "inf"], "--simplify takes a positive, finite number of voxel sides"),
    (["--simplify", "nan"], "--simplify takes a positive, finite number of voxel sides"),
    (["--simplify_keep_duplicates"], "--simplify_keep_duplicates goes with --simplify X"),
    (["--smooth", "0"], "--smooth takes a number of iterations, 1..10000"),
    (["--smooth", "10001"], "--smooth takes a number of iterations, 1..10000"),
    (["--smooth", "3", "--smooth_lambda", "0"], "--smooth_lambda takes a factor in (0, 1]"),
    (["--smooth", "3", "--smooth_lambda", "nan"], "--smooth_lambda takes a factor in (0, 1]"),
    (["--smooth", "3", "--smooth_mu", "0.1"], "--smooth_mu takes a factor in [-1, 0]"),
    (["--smooth", "3", "--smooth_mu", "-1.5"], "--smooth_mu takes a factor in [-1, 0]"),
    (["--smooth", "3", "--smooth_mu=-inf"], "--smooth_mu takes a factor in [-1, 0]"),
    (["--smooth", "3", "--smooth_max_move", "0"],
     "--smooth_max_move takes a positive number of voxel sides, or inf"),
    (["--smooth", "3", "--smooth_max_move", "nan"],
     "--smooth_max_move takes a positive number of voxel sides, or inf"),
    (["--smooth_lambda", "0.5"], "--smooth_lambda goes with --smooth N"),
    (["--smooth_mu", "-0.5"], "--smooth_mu goes with --smooth N"),
    (["--smooth_max_move", "2"], "--smooth_max_move goes with --smooth N"),
    (["--smooth_free_boundary"], "--smooth_free_boundary goes with --smooth N"),
    # the stages are checked in the order they run: the first one's error is the one reported
    (["--smooth", "0", "--simplify", "0", "--keep_largest", "0"],
     "--keep_largest takes a number of components, 1 or more"),
    (["--smooth_mu", "-0.5", "--simplify_keep_duplicates"],
     "--simplify_keep_duplicates goes with --simplify X"),
]

# render_volume without --mesh PATH: the flags are the mesh's
NO_MESH_ERRORS = [
    (["--min_component_faces", "5"],
     "--min_component_faces goes with --mesh PATH: the components are the mesh's"),
    (["--min_component_fraction", "0.5"],
     "--min_component_fraction goes with --mesh PATH: the components are the mesh's"),
    (["--keep_largest", "1"],
     "--keep_largest goes with --mesh PATH: the components are the mesh's"),
    (["--simplify", "2"], "--simplify goes with --mesh PATH: the simplification is the mesh's"),
    (["--simplify", "2", "--simplify_keep_duplicates"],
     "--simplify goes with --mesh PATH: the simplification is the mesh's"),
    (["--smooth", "3"], "--smooth goes with --mesh PATH: the smoothing is the mesh's"),
    (["--smooth", "3", "--smooth_lambda", "0.4", "--smooth_mu", "-0.45", "--smooth_max_move",
      "2", "--smooth_free_boundary"], "--smooth goes with --mesh PATH: the smoothing is the mesh's"),
    # a point cloud of the surface is no mesh file
    (["--keep_largest", "1", "--mesh_cloud", "c.ply", "--mesh_samples", "10"],
     "--keep_largest goes with --mesh PATH: the components are the mesh's"),
    # stage by stage: a stage's range errors come before its --mesh error, a later stage's after
    (["--keep_largest", "0"], "--keep_largest takes a number of components, 1 or more"),
    (["--keep_largest", "1", "--simplify", "0"],
     "--keep_largest goes with --mesh PATH: the components are the mesh's"),
    (["--simplify_keep_duplicates"], "--simplify_keep_duplicates goes with --simplify X"),
    (["--simplify", "2", "--smooth", "0"],
     "--simplify goes with --mesh PATH: the simplification is the mesh's"),
    (["--smooth_free_boundary"], "--smooth_free_boundary goes with --smooth N"),
]


def _usage_error(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        main(argv)
    err = capsys.readouterr().err
    assert err.startswith("usage: "), err
    return e.value.code, err[err.index(": error: ") + len(": error: "):]


@pytest.fixture
def occupancy(tmp_path):
    path = str(tmp_path / "occupancy.npz")
    np.savez(open(path, "wb"), belief=np.zeros((2, 2, 2), F), bbox=np.zeros(6, F),
             grid_shape=np.array([2, 2, 2], np.int32))
    return path


@pytest.mark.parametrize("argv,message", USAGE_ERRORS, ids=[" ".join(a) for a, _ in USAGE_ERRORS])
def test_every_usage_error_is_the_parents_in_both_scripts(argv, message, occupancy, tmp_path, capsys):
    from raynet_amd.scripts import fuse_depth_maps, render_volume
    out = str(tmp_path / "out.ply")
    assert _usage_error(fuse_depth_maps.main, ["scene", "predictions", out] + argv, capsys) == \
        (2, message + "\n")
    assert _usage_error(render_volume.main, ["scene", occupancy, str(tmp_path / "maps"),
                                             "--mesh", out] + argv, capsys) == (2, message + "\n")
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "maps"))


@pytest.mark.parametrize("argv,message", NO_MESH_ERRORS, ids=[" ".join(a) for a, _ in NO_MESH_ERRORS])
def test_render_volume_without_a_mesh_refuses_the_flags(argv, message, occupancy, tmp_path, capsys):
    from raynet_amd.scripts import render_volume
    assert _usage_error(render_volume.main, ["scene", occupancy, str(tmp_path / "maps")] + argv,
                        capsys) == (2, message + "\n")
    assert not os.path.exists(str(tmp_path / "maps"))


def test_the_ten_flags_in_their_order_with_their_defaults():
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags, render_volume
    want = ["min_component_faces", "min_component_fraction", "keep_largest", "simplify",
            "simplify_keep_duplicates", "smooth", "smooth_lambda", "smooth_mu", "smooth_max_move",
            "smooth_free_boundary"]
    assert list(mesh_flags.FLAGS) == want
    for script in (fuse_depth_maps, render_volume):
        actions = [a.dest for a in script.build_parser()._actions]
        at = actions.index(want[0])
        assert actions[at:at + 10] == want and actions[at - 1] in ("seed", "depth_tolerance")
        args = script.build_parser().parse_args(["a", "b", "c"])
        assert all(getattr(args, f) is None for f in want) and mesh_flags.given(args) == []
        args = script.build_parser().parse_args(["a", "b", "c", "--smooth_mu", "0", "--keep_largest", "2"])
        assert mesh_flags.given(args) == ["keep_largest", "smooth_mu"]
        assert mesh_flags.given(args, mesh_flags.SMOOTH_FLAGS) == ["smooth_mu"]


def test_apply_chains_the_stages_on_the_volumes_voxel(monkeypatch):
    from raynet_amd.scripts import mesh_flags
    volume = types.SimpleNamespace(bbox=np.array([-1.0, 0.5, 2.0, 3.0, 2.5, 2.75], F),
                                   grid_shape=(8, 4, 3))
    voxel = (volume.bbox.astype(np.float64)[3:] - volume.bbox.astype(np.float64)[:3]) / \
        np.array([8.0, 4.0, 3.0])
    assert np.array_equal(mesh_flags.voxel_sides(volume), voxel) and voxel.dtype == np.float64
    assert np.array_equal(voxel, [0.5, 0.5, 0.25])
    calls = []
    monkeypatch.setattr(mesh_flags, "drop_components",
                        lambda mesh, args: calls.append(("components", mesh, args)) or "dropped")
    monkeypatch.setattr(mesh_flags, "simplify", lambda mesh, args, voxel, origin:
                        calls.append(("simplify", mesh, args, voxel, origin)) or "simplified")
    monkeypatch.setattr(mesh_flags, "smooth", lambda mesh, args, voxel:
                        calls.append(("smooth", mesh, args, voxel)) or "smoothed")
    assert mesh_flags.apply("mesh", "args", volume) == "smoothed"
    assert [c[:3] for c in calls] == [("components", "mesh", "args"), ("simplify", "dropped", "args"),
                                      ("smooth", "simplified", "args")]
    assert np.array_equal(calls[1][3], voxel) and np.array_equal(calls[1][4], [-1.0, 0.5, 2.0])
    assert calls[1][4].dtype == np.float64 and np.array_equal(calls[2][3], voxel)


def test_without_a_flag_apply_hands_the_mesh_through():
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    volume = types.SimpleNamespace(bbox=np.array([0, 0, 0, 1, 1, 1], F), grid_shape=(2, 2, 2))
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply"])
    mesh = object()
    assert mesh_flags.apply(mesh, args, volume) is mesh


# ------------------------------------------------------------------------------ the headers
def test_the_mesh_guards_are_stated_once():
    """raynet_mesh_args.h alone defines the limits, the guards and the capped launch geometry of
    the mesh kernels; the four mesh headers import them; the scan is a file of its own and
    raynet_simplify.inl declares nothing that another file defines."""
    from raynet_amd import _lib
    define = re.compile(r"^\s*(?:constexpr|inline|enum)\b[^;(]*\b(INT32_LIMIT|MAX_BLOCKS|Verdict|"
                        r"sizes_ok|vertex_in|face_in|corner_in|clamp_slot|xyz_index|"
                        r"face_names_vertices|blocks)\b\s*[=({]", re.M)
    shared = os.path.join(CSRC, "raynet_mesh_args.h")
    text = re.sub(r"//.*", "", open(shared).read())
    assert sorted(define.findall(text)) == sorted([
        "INT32_LIMIT", "MAX_BLOCKS", "Verdict", "sizes_ok", "vertex_in", "face_in", "corner_in",
        "clamp_slot", "xyz_index", "face_names_vertices", "blocks"])
    assert "hip" not in text.lower() and not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, re.M)
    assert "namespace rn_mesh {" in text and "#pragma once" in text
    for name in ("appearance", "components", "smooth", "simplify"):
        header = re.sub(r"//.*", "", open(os.path.join(CSRC, "raynet_%s_args.h" % name)).read())
        assert '#include "raynet_mesh_args.h"' in header, name
        assert define.findall(header) == [], name
        assert "INT32_LIMIT - 1" not in header and "INT32_LIMIT / 3" not in header, name
        assert "using rn_mesh::Verdict, " in header and "sizes_ok(nv, nf)" in header, name
    # the headers with contracts of their own keep them
    for name in ("fusion", "isosurface", "volume"):
        assert "rn_mesh" not in open(os.path.join(CSRC, "raynet_%s_args.h" % name)).read(), name
    # the face predicate of the components is the shared one
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, "raynet_components_args.h")).read())
    assert "return rn_mesh::face_names_vertices(nv, a, b, c);" in code
    # the scan: its own files, included once in front of its users, listed for the rebuild
    unit = open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert unit.count('#include "raynet_scan.inl"') == 1
    assert unit.index('"raynet_scan.inl"') < unit.index('"raynet_simplify.inl"')
    assert unit.index('"raynet_scan.inl"') < unit.index('"raynet_isosurface.inl"')
    scan = re.sub(r"//.*", "", open(os.path.join(CSRC, "raynet_scan.inl")).read())
    for piece in ("scan_wave_u64(uint64_t x) {", "scan_block_u64(uint64_t x, uint64_t *total) {",
                  "void k_scan_reduce(", "void k_scan_tile(", "int scan_exclusive_u64("):
        assert scan.count(piece) == 1, piece
    for f in ("raynet_isosurface.inl", "raynet_simplify.inl"):
        code = re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())
        assert "k_scan" not in code and "scan_wave" not in code and "scan_block" not in code, f
        # every function the file names with a body-less prototype would be a forward declaration
        assert not re.search(r"^\w[\w \*]*\b\w+\([^;{]*\);\s*$", code, re.M), f
    iso = open(os.path.join(CSRC, "raynet_isosurface_args.h")).read()
    assert "SCAN_TILE" not in iso and '#include "raynet_scan_args.h"' in iso
    simplify = open(os.path.join(CSRC, "raynet_simplify_args.h")).read()
    assert "raynet_isosurface_args.h" not in simplify and "rn_iso" not in simplify
    assert "rn_scan::scan_scratch_words(" in simplify
    for f in ("raynet_mesh_args.h", "raynet_scan.inl", "raynet_scan_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f
