"""Vertex clustering, the host side (no GPU): the argument checks, the workspace layout and every
phase of the kernels (raynet_amd/csrc/raynet_simplify_args.h) as a stand-alone program under the
address and undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter --
the kernels' use of that header, the entries in the header and the ctypes table, simplify_mesh and
SurfaceMesh.simplified against tests/simplify_truth.py with the truth in place of the GPU call,
cluster_grid, unique_faces by the torch route on the CPU device, and the flags of the two
mesh-writing scripts."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import components_truth as ct
import simplify_truth as sp
import smooth_truth as st
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_checks_layout_and_phases_under_sanitizers(tmp_path):
    run_host_program("simplify", tmp_path)


def test_the_launcher_and_the_kernels_use_the_header():
    """raynet_simplify.inl decides on the header's verdict and lays the workspace out with its
    functions; the kernels call one function of the header each and add the index of the thread
    and the atomics policy (the binning also the integer sums within a wavefront): no subscript,
    no arithmetic on positions, no LDS, no floating-point atomic; the scan is the library's one;
    the header holds no HIP and no conditional."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_simplify.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "__syncthreads" not in code
    assert "while" not in code and "goto" not in code
    assert code.count("rn_sp::simplify_args(") == 1
    assert "if (verdict == rn_sp::INVALID)" in code and "if (verdict == rn_sp::EMPTY) return RN_OK;" in code
    for use in ("rn_sp::workspace_bytes(", "rn_sp::grid_of(", "rn_sp::tables_of(",
                "rn_sp::ws_scratch(", "rn_sp::blocks("):
        assert use in code, use
    assert code.count("scan_exclusive_u64(") == 2 and "k_scan" not in code     # called twice
    kernels = re.findall(r"__global__ __launch_bounds__\(BLOCK\) void (\w+)\(SimplifyArgs a\) \{\n(.*?)\n\}\n",
                         code, re.S)
    calls = {"k_simplify_clear": "rn_sp::clear_cell(", "k_simplify_bin": "rn_sp::place_vertex(",
             "k_simplify_face_flags": "rn_sp::flag_face(",
             "k_simplify_emit_vertices": "rn_sp::emit_vertex(",
             "k_simplify_emit_faces": "rn_sp::emit_face("}
    assert [k for k, _ in kernels] == list(calls)
    for name, body in kernels:
        assert body.count(calls[name]) == 1, name
        assert "[" not in body and "double" not in body and "float" not in body, name
        assert body.count("for (") == 1 and "+= stride" in body and "atomic" not in body, name
    # the binning adds within the wavefront first: every lane reaches the shuffles (the loop runs
    # on the workgroup's first item), at most 64 rounds, and the atomics are the header's five
    assert "rn_sp::vertex_in(first, a.tables.nv)" in dict(kernels)["k_simplify_bin"]
    assert dict(kernels)["k_simplify_bin"].count("add_by_cell(") == 1
    combine = re.search(r"__device__ void add_by_cell\(.*?\n\}\n", code, re.S).group(0)
    assert "round < 64 && pending" in combine and combine.count("rn_sp::add_to_cell(") == 1
    assert "atomic" not in combine and "double" not in combine and "float" not in combine
    atomics = re.findall(r"\batomic\w+", code)
    assert sorted(atomics) == ["atomicAdd", "atomicAdd", "atomicMin"], atomics
    header = open(os.path.join(CSRC, "raynet_simplify_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "while" not in hcode and "atomic" not in hcode
    assert "#pragma once" in header
    for f in ("raynet_simplify.inl", "raynet_simplify_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
    unit = open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert unit.count('#include "raynet_simplify.inl"') == 1
    for f in ("raynet_simplify.inl", "raynet_simplify_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_entries_are_declared_and_bound_with_matching_types():
    """(The types of every entry, these included, and the restype of the size entry:
    tests/test_abi.py.)"""
    from raynet_amd import _lib
    want = {
        "rn_mesh_simplify_workspace_bytes": ("int64_t", ["int64_t nv", "int64_t nf",
                                                         "const int32_t dims[3]"]),
        "rn_mesh_simplify": ("int", [
            "rn_ctx *ctx", "int64_t nv", "const float *vertices_in", "int64_t nf",
            "const int32_t *faces_in", "const double origin[3]", "const double cell[3]",
            "const int32_t dims[3]", "float *vertices_out", "int32_t *faces_out",
            "int32_t *source", "int32_t *cluster", "int64_t *counts", "void *workspace",
            "void *stream"])}
    lib = ctypes.CDLL(_lib.build())
    for name, prototype in want.items():
        assert abi_header.prototype(name) == prototype
        assert hasattr(lib, name)
    # the size entry needs no context and no GPU: the header's arithmetic
    fn = lib.rn_mesh_simplify_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, _lib.SIGNATURES["rn_mesh_simplify_workspace_bytes"]
    dims = (ctypes.c_int32 * 3)(3, 5, 7)
    assert fn(0, 0, dims) == 32 * 105
    assert fn(257, 255, dims) == (32 * 105 + 8 * 255 + 8 * 257 + 8 * 2 + 4 * 257 + 7) // 8 * 8
    assert fn(-1, 0, dims) == -1 and fn(2 ** 31 - 1, 0, dims) == -1 and fn(1, 2 ** 40, dims) == -1
    assert fn(1, 1, (ctypes.c_int32 * 3)(65536, 32768, 1)) == -1
    assert fn(1, 1, (ctypes.c_int32 * 3)(3, 0, 7)) == -1 and fn(1, 1, None) == -1


# ------------------------------------------------------------- the plumbing, on the truth's result
@pytest.fixture
def truth_call(monkeypatch):
    """raynet_amd.simplify.mesh_simplify answered by the truth, and the vertex normals by theirs:
    the plumbing without a GPU."""
    import appearance_truth as at
    from raynet_amd import appearance, simplify
    calls = []

    def fake(vertices, faces, origin, cell, dims):
        calls.append(dict(nv=len(vertices), nf=len(faces), origin=np.array(origin),
                          cell=np.array(cell), dims=np.array(dims)))
        return sp.simplify(vertices, faces, origin, cell, dims)

    def fake_normals(vertices, faces, unit=True):
        calls.append("normals")
        n = at.area_normals(vertices, faces)
        return appearance.normalized(n) if unit else n

    monkeypatch.setattr(simplify, "mesh_simplify", fake)
    monkeypatch.setattr(appearance, "vertex_normals", fake_normals)
    return calls


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_simplify_mesh_is_the_truth_on_the_grid_of_cluster_grid(truth_call):
    from raynet_amd.simplify import simplify_mesh
    vertices, faces = st.binary_ball()
    out, out_faces, source = simplify_mesh(vertices, faces, 2.0)
    grid = sp.grid_around(vertices, 2.0)
    call = truth_call[-1]
    assert np.array_equal(call["origin"], grid[0]) and np.array_equal(call["cell"], grid[1])
    assert np.array_equal(call["dims"], grid[2]) and call["dims"].dtype == np.int32
    want = sp.simplify(vertices, faces, *grid)
    assert np.array_equal(_bits(out), _bits(want[0])) and np.array_equal(source, want[2])
    assert np.array_equal(out_faces, sp.unique_faces(want[1])[0])
    assert out.dtype == F and out_faces.dtype == np.int32 and source.dtype == np.int32
    # every output vertex is still in a face: dropped duplicates name what the first one names
    assert np.array_equal(np.unique(out_faces), np.arange(len(out)))
    kept = simplify_mesh(vertices, faces, 2.0, drop_duplicate_faces=False)
    assert np.array_equal(kept[1], want[1])
    # three cells, an origin, lists and tensors
    import torch
    got = simplify_mesh(torch.from_numpy(vertices), faces.tolist(), (1.0, 2.0, 3.0),
                        origin=(-0.25, -0.5, -0.75))
    call = truth_call[-1]
    assert np.array_equal(call["origin"], [-0.25, -0.5, -0.75])
    assert np.array_equal(call["cell"], [1.0, 2.0, 3.0])
    want = sp.simplify(vertices, faces, call["origin"], call["cell"], call["dims"])
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    # the refusals name the argument, and nothing reaches the GPU call
    n = len(truth_call)
    for kw, match in [(dict(cell=0.0), "cell"), (dict(cell=-1.0), "cell"),
                      (dict(cell=float("nan")), "cell"), (dict(cell=float("inf")), "cell"),
                      (dict(cell=(1.0, 2.0)), "cell"), (dict(cell=(1.0, 0.0, 1.0)), "cell"),
                      (dict(cell=1e-4), "cell"),
                      (dict(cell=1.0, origin=(0.0, float("nan"), 0.0)), "origin"),
                      (dict(cell=1.0, origin=(0.0, 1.0)), "origin"),
                      (dict(cell=1.0, faces=np.array([[0, 1, len(vertices)]])), "faces"),
                      (dict(cell=1.0, faces=np.array([[0, -1, 2]])), "faces")]:
        args = dict(vertices=vertices, faces=faces)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            simplify_mesh(**args)
    assert len(truth_call) == n


def test_without_a_gpu_there_is_no_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from raynet_amd import _lib
    from raynet_amd.simplify import simplify_mesh
    vertices, faces = st.strip(10, 1)
    with pytest.raises(_lib.RaynetHipError):
        simplify_mesh(vertices, faces, 1.0)


def test_surface_mesh_simplified_takes_colours_by_source_and_normals_only_if_present(truth_call):
    import appearance_truth as at
    from raynet_amd import appearance
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = st.binary_ball()
    nv = len(vertices)
    rng = np.random.default_rng(1)
    colors = rng.integers(0, 256, size=(nv, 3)).astype(np.uint8)
    stale = rng.normal(size=(nv, 3)).astype(F)
    want = sp.simplify(vertices, faces, *sp.grid_around(vertices, 2.0))
    want_faces = sp.unique_faces(want[1])[0]
    mesh = SurfaceMesh(vertices, faces)
    out = mesh.simplified(2.0)
    assert out is not mesh and np.array_equal(_bits(out.vertices), _bits(want[0]))
    assert np.array_equal(out.faces, want_faces) and len(out.faces) * 3 <= len(faces)
    assert out.normals is None and out.colors is None and "normals" not in truth_call
    assert np.array_equal(_bits(mesh.vertices), _bits(vertices)) and np.array_equal(mesh.faces, faces)
    out = SurfaceMesh(vertices, faces, colors=colors).simplified(2.0)
    assert np.array_equal(out.colors, colors[want[2]]) and out.normals is None
    assert "normals" not in truth_call
    mesh = SurfaceMesh(vertices, faces, stale, colors)
    out = mesh.simplified(2.0)
    assert truth_call[-1] == "normals"
    assert np.array_equal(_bits(out.normals),
                          _bits(appearance.normalized(at.area_normals(want[0], want_faces))))
    assert np.array_equal(out.colors, colors[want[2]]) and np.array_equal(_bits(mesh.normals), _bits(stale))
    # the keywords are simplify_mesh's own
    out = mesh.simplified((2.0, 1.0, 2.0), (-1.0, -1.0, -1.0), False)
    call = truth_call[-2]
    assert np.array_equal(call["origin"], [-1.0] * 3) and np.array_equal(call["cell"], [2.0, 1.0, 2.0])
    assert np.array_equal(out.faces, sp.simplify(vertices, faces, call["origin"], call["cell"],
                                                 call["dims"])[1])
    with pytest.raises(ValueError, match="cell"):
        mesh.simplified(0.0)
    # everything in one cell: an empty mesh, with the attributes it had
    gone = mesh.simplified(1000.0)
    assert gone.empty and len(gone.vertices) == 0 and gone.normals.shape == (0, 3)
    assert gone.colors.shape == (0, 3)


def test_an_empty_mesh_stays_empty_without_the_gpu(truth_call):
    from raynet_amd.volume import SurfaceMesh
    loose = st.positions(4, 2)
    for mesh in (SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)),
                 SurfaceMesh(loose, np.zeros((0, 3), np.int32), loose, np.zeros((4, 3), np.uint8))):
        out = mesh.simplified(1.0)
        assert out is not mesh and out.empty and out.faces.shape == (0, 3)
        assert np.array_equal(_bits(out.vertices), _bits(mesh.vertices))
        assert (out.normals is None) == (mesh.normals is None)
        assert (out.colors is None) == (mesh.colors is None)
        with pytest.raises(ValueError, match="cell"):
            mesh.simplified(-1.0)
    assert truth_call == []


def test_cluster_grid_anchors_at_multiples_of_the_cell_and_refuses_huge_tables():
    from raynet_amd.simplify import CELL_BYTES, MAX_CELLS, cluster_grid
    assert MAX_CELLS == 2 ** 28 and CELL_BYTES == 32
    vertices, _ = st.binary_ball()
    for cell in (0.5, 2.0, (0.7, 1.3, 2.9)):
        origin, cell3, dims = cluster_grid(vertices, cell)
        want = sp.grid_around(vertices, cell)
        assert np.array_equal(origin, want[0]) and np.array_equal(cell3, want[1])
        assert np.array_equal(dims, want[2]) and dims.dtype == np.int32 and origin.dtype == np.float64
        # every vertex is binned, the last cell of every axis is needed
        c, q, _ = sp.cells_of(vertices, origin, cell3, dims)
        assert (c >= 0).all() and np.array_equal(q.max(0) + 1, dims)
        assert np.allclose(origin / cell3, np.rint(origin / cell3))
    # a translated crop clusters the same way: the same world cells
    shift = np.array([4.0, -6.0, 10.0])
    a = cluster_grid(vertices, 2.0)
    b = cluster_grid(vertices[: len(vertices) // 2] + shift.astype(F), 2.0)
    assert np.allclose((b[0] - a[0]) / 2.0, np.rint((b[0] - a[0]) / 2.0))
    # an origin of the caller's; dims cover the maximum and are at least 1
    origin, _, dims = cluster_grid(vertices, 4.0, origin=(-3.0, 0.0, 100.0))
    assert np.array_equal(origin, [-3.0, 0.0, 100.0]) and dims[2] == 1
    assert dims[0] == int(np.floor((vertices[:, 0].max() + 3.0) / 4.0)) + 1
    # non-finite coordinates play no part; nothing finite: one cell at 0
    bad = np.array(vertices, F)
    bad[3], bad[5, 1] = np.nan, np.inf
    ok = np.isfinite(bad)
    got = cluster_grid(bad, 2.0)
    for k in range(3):
        x = bad[:, k][ok[:, k]].astype(np.float64)
        assert got[0][k] == np.floor(x.min() / 2.0) * 2.0
    got = cluster_grid(np.full((4, 3), np.nan, F), 2.0)
    assert np.array_equal(got[0], [0.0] * 3) and np.array_equal(got[2], [1, 1, 1])
    assert np.array_equal(cluster_grid(np.zeros((0, 3), F), 2.0)[2], [1, 1, 1])
    # 2^28 cells are taken, one more is not
    span = np.array([[0.0, 0.0, 0.0], [1023.5, 511.5, 511.5]], F)
    assert int(np.prod(cluster_grid(span, 1.0)[2].astype(np.int64))) == 2 ** 28
    with pytest.raises(ValueError, match="cell"):
        cluster_grid(np.array([[0.0, 0.0, 0.0], [1024.5, 511.5, 511.5]], F), 1.0)
    with pytest.raises(ValueError, match="cell"):
        cluster_grid(np.array([[0.0, 0.0, 0.0], [1e30, 1.0, 1.0]], F), 1.0)


def test_unique_faces_by_the_torch_route_is_the_dictionarys():
    import torch
    from raynet_amd.simplify import unique_faces
    vertices, faces = st.binary_ball()
    clustered = sp.simplify(vertices, faces, *sp.grid_around(vertices, 2.0))[1]
    thin = sp.simplify(vertices, faces, *sp.grid_around(vertices, 6.0))[1]
    cases = [clustered, thin, np.concatenate([clustered, clustered[::-1, ::-1]]),
             np.concatenate([thin[:, [1, 2, 0]], thin]), ct.strip(40), ct.star(9)[0],
             ct.tetrahedra(3)[0], np.zeros((0, 3), np.int32),
             np.array([[0, 1, 2], [2, 0, 1], [2, 1, 0], [0, 1, 3], [1, 0, 2]], np.int32),
             np.array([[2 ** 31 - 1, 0, -2 ** 31], [-2 ** 31, 2 ** 31 - 1, 0], [5, 5, 5]], np.int32)]
    assert len(cases) == 10
    assert len(sp.unique_faces(thin)[0]) < len(thin)          # there are doubles to find
    for faces in cases:
        want, _ = sp.unique_faces(faces)
        got = unique_faces(torch.from_numpy(np.ascontiguousarray(faces, np.int32)))
        assert got.dtype == torch.int32 and got.device.type == "cpu"
        assert np.array_equal(got.numpy(), want.reshape(-1, 3))
        assert np.array_equal(unique_faces(np.asarray(faces, np.int64)).numpy(), want.reshape(-1, 3))


# ------------------------------------------------------------------------------ the scripts
def test_the_flag_helper_simplifies_and_reports(truth_call, capsys, tmp_path):
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = st.binary_ball()
    mesh = SurfaceMesh(vertices, faces)
    voxel, corner = np.array([0.5, 0.25, 1.0]), np.array([-0.5, -0.5, -0.5])
    # without --simplify: the very object, nothing printed, and so the bytes of the file
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply"])
    assert mesh_flags.given(args) == []
    assert mesh_flags.simplify(mesh, args, voxel, corner) is mesh and capsys.readouterr().out == ""
    assert truth_call == []
    before, after = str(tmp_path / "before.ply"), str(tmp_path / "after.ply")
    mesh.save_ply(before)
    mesh_flags.simplify(mesh, args, voxel, corner).save_ply(after)
    assert open(before, "rb").read() == open(after, "rb").read()
    # --simplify 2.5: cells of 2.5 voxel sides per axis, anchored at the box's minimum -- whole
    # cells in front of it where the closed surface reaches out of the box
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--simplify", "2.5"])
    assert mesh_flags.given(args) == ["simplify"]
    out = mesh_flags.simplify(mesh, args, voxel, corner)
    call = truth_call[-1]
    assert np.array_equal(call["cell"], 2.5 * voxel)
    steps = (call["origin"] - corner) / call["cell"]
    assert np.array_equal(steps, np.rint(steps)) and (steps <= 0).all() and (steps >= -1).all()
    assert (call["origin"] <= vertices.min(0)).all()
    want = sp.simplify(vertices, faces, call["origin"], call["cell"], call["dims"])
    want_faces = sp.unique_faces(want[1])[0]
    assert np.array_equal(_bits(out.vertices), _bits(want[0])) and np.array_equal(out.faces, want_faces)
    assert capsys.readouterr().out == \
        "simplify: cell 2.5 voxel sides, %d -> %d vertices, %d -> %d faces\n" % (
            len(vertices), len(want[0]), len(faces), len(want_faces))
    # every flag: a collapsed two-sided sheet keeps both of its sides
    sheet = SurfaceMesh(*sp.thin_sheet())
    quarter = np.array([0.25, 0.25, 0.25])
    args = fuse_depth_maps.build_parser().parse_args(
        ["s", "p", "o.ply", "--simplify", "2", "--simplify_keep_duplicates"])
    assert mesh_flags.given(args) == ["simplify", "simplify_keep_duplicates"]
    out = mesh_flags.simplify(sheet, args, quarter, np.zeros(3))
    call = truth_call[-1]
    assert np.array_equal(call["cell"], [0.5] * 3) and np.array_equal(call["origin"], [0.0] * 3)
    want = sp.simplify(sheet.vertices, sheet.faces, call["origin"], call["cell"], call["dims"])
    single = sp.unique_faces(want[1])[0]
    assert np.array_equal(out.faces, want[1]) and 0 < len(single) == len(want[1]) // 2
    assert "simplify: cell 2 voxel sides, " in capsys.readouterr().out
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--simplify", "2"])
    assert np.array_equal(mesh_flags.simplify(sheet, args, quarter, np.zeros(3)).faces, single)


def test_the_scripts_know_the_flags_and_refuse_bad_values(tmp_path, capsys):
    from raynet_amd.scripts import fuse_depth_maps, render_volume
    out = str(tmp_path / "out.ply")
    occupancy = str(tmp_path / "occupancy.npz")
    np.savez(open(occupancy, "wb"), belief=np.zeros((2, 2, 2), F), bbox=np.zeros(6, F),
             grid_shape=np.array([2, 2, 2], np.int32))
    cases = [(fuse_depth_maps, ["scene", "predictions", out], []),
             (render_volume, ["scene", occupancy, str(tmp_path / "maps")], ["--mesh", out])]
    for script, positional, mesh_flag in cases:
        a = script.build_parser().parse_args(positional)
        assert a.simplify is None and not a.simplify_keep_duplicates
        a = script.build_parser().parse_args(positional + ["--simplify", "2.5",
                                                           "--simplify_keep_duplicates"])
        assert (a.simplify, a.simplify_keep_duplicates) == (2.5, True)
        for argv, message in [(["--simplify", "0"], "--simplify"), (["--simplify", "-2"], "--simplify"),
                              (["--simplify", "nan"], "--simplify"), (["--simplify", "inf"], "--simplify"),
                              (["--simplify_keep_duplicates"], "--simplify_keep_duplicates")]:
            with pytest.raises(SystemExit) as e:
                script.main(positional + mesh_flag + argv)
            assert e.value.code == 2
            assert message in capsys.readouterr().err, (script.__name__, argv)
    # render_volume: the flags are the mesh's
    for argv, message in [(["--simplify", "2"], "--simplify"),
                          (["--simplify", "2", "--simplify_keep_duplicates", "--mesh_cloud", out,
                            "--mesh_samples", "10"], "--simplify")]:
        with pytest.raises(SystemExit) as e:
            render_volume.main(cases[1][1] + argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err and "--mesh" in err, argv
    assert not os.path.exists(out)
    # the stage runs between the component filter and the smoothing
    import inspect
    from raynet_amd.scripts import mesh_flags
    stages = inspect.getsource(mesh_flags.apply)
    assert stages.index("drop_components(") < stages.index("simplify(") < stages.index("smooth(")
    for script in (fuse_depth_maps, render_volume):
        body = inspect.getsource(script.main)
        assert body.index("mesh_flags.apply(") < body.index("compute_normals()")
