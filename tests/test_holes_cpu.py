"""Hole filling, the host side (no GPU): the argument checks, the workspace layout and every phase
of the kernels (raynet_amd/csrc/raynet_holes_args.h) as a stand-alone program under the address and
undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter -- the kernels'
use of that header, the entries in the header and the ctypes table, fill_holes and
SurfaceMesh.filled against tests/holes_truth.py with the truth in place of the GPU call, and the
flag of the two mesh-writing scripts."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import holes_truth as ht
import abi_header
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def test_checks_layout_and_phases_under_sanitizers(tmp_path):
    run_host_program("holes", tmp_path)


def test_the_launcher_and_the_kernels_use_the_header():
    """raynet_holes.inl decides on the header's verdict and lays the workspace out with its
    functions; every kernel is one grid-stride loop around one function of the header (the
    flattening: the union-find's) and adds the index of the thread and the atomics policies (the
    tally also the integer sums within a wavefront): no floating point, no LDS; integer atomics only; the union-find, its atomics and the
    scan are the library's, defined elsewhere; the header holds no HIP and no conditional."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_holes.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "__syncthreads" not in code
    assert "while" not in code and "goto" not in code
    assert code.count("rn_hl::fill_args(") == 1
    assert "if (verdict == rn_hl::INVALID)" in code and "if (verdict == rn_hl::EMPTY) return RN_OK;" in code
    for use in ("rn_hl::workspace_bytes(", "rn_hl::tables_of(", "rn_hl::ws_scratch(", "rn_hl::blocks("):
        assert use in code, use
    assert code.count("scan_exclusive_u64(") == 1 and "k_scan" not in code
    kernels = re.findall(r"__global__ __launch_bounds__\(BLOCK\) void (\w+)\(HolesArgs a\) \{\n(.*?)\n\}\n",
                         code, re.S)
    calls = {"k_holes_init": "rn_hl::init_vertex(", "k_holes_edges": "rn_hl::mark_edge(",
             "k_holes_flatten": "rn_cc::flatten(", "k_holes_tally": "rn_hl::tally_of(",
             "k_holes_flags": "rn_hl::flag_vertex(", "k_holes_emit": "rn_hl::emit_loop("}
    assert [k for k, _ in kernels] == list(calls)
    for name, body in kernels:
        assert body.count(calls[name]) == 1, name
        assert "double" not in body and "float" not in body and "atomic" not in body, name
        assert body.count("for (") == 1 and "+= stride" in body, name
        assert set(re.findall(r"\w+\[[^\]]*\]", body)) <= {"status[0]"}, name     # no other subscript
    # the tally adds within the wavefront first, through the components' add_by_label: every lane
    # reaches the shuffles (the loop runs on the workgroup's first item); the flags add into the
    # partial sums of the workgroup's slot, which the launcher clears
    bodies = dict(kernels)
    assert "rn_hl::corner_in(first, a.tables.nf)" in bodies["k_holes_tally"]
    assert bodies["k_holes_tally"].count("add_by_label(") == 2 and "void add_by_label(" not in code
    assert "blockIdx.x % rn_hl::SLOTS" in bodies["k_holes_flags"] and "__shfl" not in code
    assert "hipMemsetAsync(t.partial, 0, (size_t)rn_hl::partial_bytes(), S(stream))" in code
    assert sorted(set(re.findall(r"\batomic\w+", code))) == ["atomicAdd", "atomicMin"]
    # reused, not redefined
    for name in ("struct AgentAtomics", "find(", "unite(", "scan_wave", "scan_block"):
        assert name not in code, name
    assert "const AgentAtomics uf{a.tables.parent};" in code
    components = open(os.path.join(CSRC, "raynet_components.inl")).read()
    assert components.count("struct AgentAtomics {") == 1
    header = open(os.path.join(CSRC, "raynet_holes_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "while" not in hcode and "atomic" not in hcode.lower()
    assert "#pragma once" in header and '#include "raynet_mesh_args.h"' in header
    assert '#include "raynet_components_args.h"' in header and "rn_scan::scan_scratch_words(" in header
    assert "using rn_mesh::Verdict, " in header and "sizes_ok(nv, nf)" in header
    assert "rn_cc::unite(uf, " in hcode and "constexpr int32_t find(" not in hcode
    define = re.compile(r"^\s*(?:constexpr|inline|enum)\b[^;(]*\b(INT32_LIMIT|MAX_BLOCKS|Verdict|"
                        r"sizes_ok|vertex_in|face_in|corner_in|clamp_slot|xyz_index|"
                        r"face_names_vertices|blocks)\b\s*[=({]", re.M)
    assert define.findall(hcode) == []
    # the proof the header has to state
    for words in ("No loop waits, every chase is bounded", "exactly E <= max_edges steps",
                  "parent[x] <= x at all times"):
        assert words in header, words
    for f in ("raynet_holes.inl", "raynet_holes_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
    unit = open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert unit.count('#include "raynet_holes.inl"') == 1
    assert unit.index('"raynet_scan.inl"') < unit.index('"raynet_holes.inl"')
    assert unit.index('"raynet_components.inl"') < unit.index('"raynet_holes.inl"')
    for f in ("raynet_holes.inl", "raynet_holes_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_entries_are_declared_and_bound_with_matching_types():
    """(The types of every entry, these included, and the restype of the size entry:
    tests/test_abi.py.)"""
    from raynet_amd import _lib
    want = {
        "rn_mesh_fill_holes_workspace_bytes": ("int64_t", ["int64_t nv", "int64_t nf"]),
        "rn_mesh_fill_holes": ("int", [
            "rn_ctx *ctx", "int64_t nv", "const float *vertices", "int64_t nf",
            "const int32_t *faces", "const int32_t *offsets", "const int32_t *corners",
            "int32_t max_edges", "float *new_vertices", "int32_t *new_faces", "int32_t *source",
            "int64_t *counts", "void *workspace", "void *stream"])}
    lib = ctypes.CDLL(_lib.build())
    for name, prototype in want.items():
        assert abi_header.prototype(name) == prototype
        assert hasattr(lib, name)
    # the size entry needs no context and no GPU: the header's arithmetic
    fn = lib.rn_mesh_fill_holes_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_int64, _lib.SIGNATURES["rn_mesh_fill_holes_workspace_bytes"]
    assert fn(0, 0) == 16 + 6144
    assert fn(257, 255) == (8 * 257 + 8 * 2 + 8 + 6144 + 24 * 257 + 8 + 3 * 255 + 7) // 8 * 8
    assert fn(-1, 0) == -1 and fn(2 ** 31 - 1, 0) == -1 and fn(1, 2 ** 40) == -1
    assert fn(2 ** 31 - 2, 0) > 0 and fn(2 ** 31 - 2, 1) == -1


# ------------------------------------------------------------- the plumbing, on the truth's result
@pytest.fixture
def truth_call(monkeypatch):
    """raynet_amd.holes.mesh_fill_holes answered by the truth, and the vertex normals by theirs:
    the plumbing without a GPU."""
    import appearance_truth as at
    from raynet_amd import appearance, holes
    calls = []

    def fake(vertices, faces, max_edges):
        calls.append(dict(nv=len(vertices), nf=len(faces), max_edges=max_edges))
        assert vertices.dtype == F and faces.dtype == np.int32 and isinstance(max_edges, int)
        return ht.fill(vertices, faces, max_edges)

    def fake_normals(vertices, faces, unit=True):
        calls.append("normals")
        n = at.area_normals(vertices, faces)
        return appearance.normalized(n) if unit else n

    monkeypatch.setattr(holes, "mesh_fill_holes", fake)
    monkeypatch.setattr(appearance, "vertex_normals", fake_normals)
    return calls


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_fill_holes_appends_the_caps_and_names_what_it_refuses(truth_call):
    import torch
    from raynet_amd.holes import COUNTS, fill_holes
    assert COUNTS == ht.COUNTS
    vertices, faces = ht.punched_sheet()
    out_v, out_f, source, stats = fill_holes(vertices, faces, 10)
    want = ht.filled_mesh(vertices, faces, 10)
    assert truth_call[-1] == dict(nv=len(vertices), nf=len(faces), max_edges=10)
    assert np.array_equal(_bits(out_v), _bits(want[0])) and np.array_equal(out_f, want[1])
    assert np.array_equal(source, [28, 48, 71]) and stats == want[3]
    assert stats == dict(filled=3, new_faces=16, loops=4, not_simple=0, boundary_edges=58)
    assert out_v.dtype == F and out_f.dtype == np.int32 and source.dtype == np.int32
    # the input comes first, with its bits
    assert np.array_equal(_bits(out_v[:len(vertices)]), _bits(vertices))
    assert np.array_equal(out_f[:len(faces)], faces)
    # lists and tensors
    got = fill_holes(torch.from_numpy(vertices), faces.tolist(), np.int64(42))
    assert got[3]["filled"] == 4 and truth_call[-1]["max_edges"] == 42
    # nothing to do: no GPU call
    n = len(truth_call)
    empty = fill_holes(np.zeros((0, 3), F), np.zeros((0, 3), np.int32), 3)
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3) and empty[3]["loops"] == 0
    loose = fill_holes(vertices, np.zeros((0, 3), np.int32), 3)
    assert np.array_equal(_bits(loose[0]), _bits(vertices)) and len(loose[2]) == 0
    # the refusals name the argument, and nothing reaches the GPU call
    for kw, match in [(dict(max_edges=2), "max_edges"), (dict(max_edges=0), "max_edges"),
                      (dict(max_edges=-5), "max_edges"), (dict(max_edges=65537), "max_edges"),
                      (dict(max_edges=3.5), "max_edges"), (dict(max_edges=True), "max_edges"),
                      (dict(faces=np.array([[0, 1, len(vertices)]])), "faces"),
                      (dict(faces=np.array([[0, -1, 2]])), "faces")]:
        args = dict(vertices=vertices, faces=faces, max_edges=10)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            fill_holes(**args)
    assert len(truth_call) == n
    for ok in (3, 65536, 10.0):
        fill_holes(vertices, faces, ok)


def test_without_a_gpu_there_is_no_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from raynet_amd import _lib
    from raynet_amd.holes import fill_holes
    vertices, faces = ht.open_tetrahedron()
    with pytest.raises(_lib.RaynetHipError):
        fill_holes(vertices, faces, 3)


def test_surface_mesh_filled_takes_colours_by_source_and_normals_only_if_present(truth_call):
    import appearance_truth as at
    from raynet_amd import appearance
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = ht.punched_sheet()
    nv = len(vertices)
    rng = np.random.default_rng(1)
    colors = rng.integers(0, 256, size=(nv, 3)).astype(np.uint8)
    stale = rng.normal(size=(nv, 3)).astype(F)
    want = ht.filled_mesh(vertices, faces, 10)
    mesh = SurfaceMesh(vertices, faces)
    out = mesh.filled(10)
    assert out is not mesh and np.array_equal(_bits(out.vertices), _bits(want[0]))
    assert np.array_equal(out.faces, want[1]) and out.normals is None and out.colors is None
    assert "normals" not in truth_call
    assert np.array_equal(_bits(mesh.vertices), _bits(vertices)) and np.array_equal(mesh.faces, faces)
    out, stats = SurfaceMesh(vertices, faces, colors=colors).filled(10, return_stats=True)
    assert stats == want[3] and out.normals is None and "normals" not in truth_call
    assert np.array_equal(out.colors[:nv], colors) and np.array_equal(out.colors[nv:], colors[[28, 48, 71]])
    mesh = SurfaceMesh(vertices, faces, stale, colors)
    out = mesh.filled(10)
    assert truth_call[-1] == "normals"
    assert np.array_equal(_bits(out.normals),
                          _bits(appearance.normalized(at.area_normals(want[0], want[1]))))
    assert np.array_equal(_bits(mesh.normals), _bits(stale)) and len(out.colors) == nv + 3
    with pytest.raises(ValueError, match="max_edges"):
        mesh.filled(2)


def test_an_empty_mesh_stays_empty_without_the_gpu(truth_call):
    from raynet_amd.volume import SurfaceMesh
    loose = ht.punched_sheet()[0][:4]
    for mesh in (SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)),
                 SurfaceMesh(loose, np.zeros((0, 3), np.int32), loose, np.zeros((4, 3), np.uint8))):
        out, stats = mesh.filled(10, return_stats=True)
        assert out is not mesh and out.empty and out.faces.shape == (0, 3)
        assert np.array_equal(_bits(out.vertices), _bits(mesh.vertices))
        assert (out.normals is None) == (mesh.normals is None)
        assert (out.colors is None) == (mesh.colors is None)
        assert stats == dict.fromkeys(ht.COUNTS, 0)
        with pytest.raises(ValueError, match="max_edges"):
            mesh.filled(65537)
    assert truth_call == []


# ------------------------------------------------------------------------------ the scripts
def test_the_flag_helper_fills_and_reports(truth_call, capsys, tmp_path):
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = ht.bow_tie_sheet()
    mesh = SurfaceMesh(vertices, faces)
    # without --fill_holes: the very object, nothing printed, and so the bytes of the file
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply"])
    assert args.fill_holes is None and mesh_flags.given(args) == []
    assert mesh_flags.fill_holes(mesh, args) is mesh and capsys.readouterr().out == ""
    assert mesh_flags.fill_holes(mesh, "a namespace without the flag") is mesh
    assert truth_call == []
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--fill_holes", "10"])
    assert args.fill_holes == 10 and mesh_flags.given(args) == []
    assert mesh_flags.given(args, mesh_flags.HOLE_FLAGS) == ["fill_holes"]
    out = mesh_flags.fill_holes(mesh, args)
    want = ht.filled_mesh(vertices, faces, 10)
    assert np.array_equal(_bits(out.vertices), _bits(want[0])) and np.array_equal(out.faces, want[1])
    assert capsys.readouterr().out == \
        "holes: 3 loops, 1 filled (1 not simple, 1 longer than 10), %d -> %d faces\n" % (
            len(faces), len(faces) + 4)
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--fill_holes", "32"])
    mesh_flags.fill_holes(mesh, args)
    assert capsys.readouterr().out == \
        "holes: 3 loops, 2 filled (1 not simple, 0 longer than 32), %d -> %d faces\n" % (
            len(faces), len(faces) + 36)


def test_the_scripts_know_the_flag_and_refuse_bad_values(tmp_path, capsys):
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags, render_volume
    assert mesh_flags.HOLE_FLAGS == ("fill_holes",) and "fill_holes" not in mesh_flags.FLAGS
    out = str(tmp_path / "out.ply")
    occupancy = str(tmp_path / "occupancy.npz")
    np.savez(open(occupancy, "wb"), belief=np.zeros((2, 2, 2), F), bbox=np.zeros(6, F),
             grid_shape=np.array([2, 2, 2], np.int32))
    cases = [(fuse_depth_maps, ["scene", "predictions", out], []),
             (render_volume, ["scene", occupancy, str(tmp_path / "maps")], ["--mesh", out])]
    for script, positional, mesh_flag in cases:
        actions = [a.dest for a in script.build_parser()._actions]
        assert actions[actions.index("smooth_free_boundary") + 1] == "fill_holes"
        for n in ("2", "0", "-1", "65537"):
            with pytest.raises(SystemExit) as e:
                script.main(positional + mesh_flag + ["--fill_holes", n])
            assert e.value.code == 2
            assert "--fill_holes takes a number of edges, 3..65536" in capsys.readouterr().err
        with pytest.raises(SystemExit) as e:
            script.main(positional + mesh_flag + ["--fill_holes", "many"])
        assert e.value.code == 2 and "--fill_holes" in capsys.readouterr().err
        # stage by stage: the components' error first, the holes' before the simplification's
        for argv, message in [(["--fill_holes", "2", "--keep_largest", "0"], "--keep_largest takes"),
                              (["--fill_holes", "2", "--simplify", "0"], "--fill_holes takes")]:
            with pytest.raises(SystemExit) as e:
                script.main(positional + mesh_flag + argv)
            assert e.value.code == 2 and message in capsys.readouterr().err
    # render_volume: the flag is the mesh's
    for argv in (["--fill_holes", "40"],
                 ["--fill_holes", "40", "--mesh_cloud", out, "--mesh_samples", "10"]):
        with pytest.raises(SystemExit) as e:
            render_volume.main(cases[1][1] + argv)
        assert e.value.code == 2
        assert "--fill_holes goes with --mesh PATH: the holes are the mesh's" in capsys.readouterr().err
    assert not os.path.exists(out)
    # the stage runs after the component filter and before the simplification and the smoothing
    stages = inspect.getsource(mesh_flags.apply)
    assert stages.index("drop_components(") < stages.index("fill_holes(") < stages.index("simplify(") \
        < stages.index("smooth(")
    for script in (fuse_depth_maps, render_volume):
        body = inspect.getsource(script.main)
        assert body.index("mesh_flags.apply(") < body.index("compute_normals()")
    for text in (mesh_flags.__doc__, open(os.path.join(REPO, "README.md")).read()):
        assert "--fill_holes" in text


def test_apply_runs_the_stage_between_the_components_and_the_simplification(truth_call, monkeypatch, capsys):
    import types
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = ht.punched_sheet()
    volume = types.SimpleNamespace(bbox=np.array([0, 0, -1, 12, 9, 1], F), grid_shape=(12, 9, 2))
    seen = []
    monkeypatch.setattr(mesh_flags, "drop_components",
                        lambda mesh, args: seen.append(("components", len(mesh.faces))) or mesh)
    monkeypatch.setattr(mesh_flags, "simplify", lambda mesh, args, voxel, origin:
                        seen.append(("simplify", len(mesh.faces))) or mesh)
    monkeypatch.setattr(mesh_flags, "smooth", lambda mesh, args, voxel:
                        seen.append(("smooth", len(mesh.faces))) or mesh)
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--fill_holes", "10"])
    out = mesh_flags.apply(SurfaceMesh(vertices, faces), args, volume)
    assert seen == [("components", len(faces)), ("simplify", len(faces) + 16), ("smooth", len(faces) + 16)]
    assert len(out.faces) == len(faces) + 16 and capsys.readouterr().out.startswith("holes: 4 loops, 3 filled")
