"""Quadric-error placement, the host side (no GPU): the argument checks, the workspace layout and
all four phases of the kernels (raynet_amd/csrc/raynet_quadric_args.h) as a stand-alone program
under the address and undefined-behaviour sanitizers, held to the values tests/quadric_truth.py
gives -- nothing sanitised is loaded into this interpreter -- the kernels' use of that header, the
entries in the header and the ctypes table, simplify_mesh and SurfaceMesh.simplified with
placement="quadric" with the truths in place of both GPU calls, and the two flags of the
mesh-writing scripts."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import quadric_truth as qt
import simplify_truth as sp
import smooth_truth as st
import abi_header
from conftest import REPO
from host_program import run_host_program

F = np.float32
D = np.float64
I = np.int32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


# ------------------------------------------------------------------------ the host program
def garbage_case():
    """A ridge strip clustered at cells of 1, then spoiled: face indices out of range, NaN and
    infinite vertices, a face without area, cluster entries of -1 and beyond nvo, a position far
    from its members, a huge triangle (weight 1) and one so small that its terms round to 0 ->
    (vertices, faces, cluster, positions, cell)."""
    vertices, faces = qt.ridge_strip(80, seed=3)
    grid = sp.grid_around(vertices, 1.0)
    mean = sp.simplify(vertices, faces, *grid)
    vertices, faces = vertices.copy(), faces.copy()
    cluster, positions = mean[3].copy(), mean[0].copy()
    nv, nvo = len(vertices), len(positions)
    faces[3, 1], faces[9, 0], faces[14, 2], faces[20, 1] = -1, nv, 2 ** 31 - 1, -2 ** 31
    faces[25] = [30, 30, 31]
    vertices[40, 1], vertices[44, 0], vertices[48, 2] = np.nan, np.inf, -np.inf
    cluster[5], cluster[6], cluster[60], cluster[61] = -1, nvo, 2 ** 31 - 1, -2 ** 31
    shared = np.flatnonzero(np.bincount(cluster[(cluster >= 0) & (cluster < nvo)],
                                        minlength=nvo) >= 2)    # still of two members or more
    positions[shared[2]] += F(40.0)                     # |r| > 2: its faces add nothing
    positions[shared[4], 1] = np.nan
    extra = np.array([[0.0, 0.0, 0.0], [3e4, 0.0, 0.0], [0.0, 3e4, 0.0],         # huge
                      [10.5, 0.25, 1.75], [10.5 + 1e-5, 0.25, 1.75], [10.5, 0.25 + 1e-5, 1.75]], F)
    assert (extra[3] != extra[4]).any() and (extra[3] != extra[5]).any()
    more = np.array([[nv, nv + 1, nv + 2], [nv + 3, nv + 4, nv + 5]], I)
    near = int(np.argmin(np.abs(mean[0].astype(D) - extra[3]).max(1)))
    assert near not in (0, shared[2], shared[4]) and np.abs(mean[0][near] - extra[3]).max() < 1.0
    cluster = np.concatenate([cluster, np.array([0, 0, 0, near, near, near], I)])
    return (np.concatenate([vertices, extra]), np.concatenate([faces, more]), cluster, positions,
            np.ones(3))


def host_cases():
    """(name, vertices, faces, cluster, positions, cell [3], regularization, max_move)."""
    tetra = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    tetra_faces = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], I)
    cube, cube_faces = qt.rotated_cube(6)
    grid = sp.grid_around(cube, 0.4)
    mean = sp.simplify(cube, cube_faces, *grid)
    flat, flat_faces = qt.flat_square()
    flat_grid = sp.grid_around(flat, 1.0)
    flat_mean = sp.simplify(flat, flat_faces, *flat_grid)
    cases = [
        ("tetrahedron", tetra, tetra_faces, np.array([0, 0, 1, 2], I),
         np.array([[0.5, 0, 0], [0, 1, 0], [0, 0, 1]], F), np.array([1.0, 0.5, 2.0]), 2.0 ** -10, 1.0),
        ("tetrahedron in one cluster", tetra, tetra_faces, np.zeros(4, I),
         np.array([[0.25, 0.25, 0.25]], F), np.ones(3), 2.0 ** -20, 1e300),
        ("cube", cube, cube_faces, mean[3], mean[0], grid[1], 2.0 ** -10, 1.0),
        ("cube held", cube, cube_faces, mean[3], mean[0], grid[1], 1.0, 1.0),
        ("cube clamped", cube, cube_faces, mean[3], mean[0], grid[1], 2.0 ** -10, 0.05),
        ("flat", flat, flat_faces, flat_mean[3], flat_mean[0], flat_grid[1], 2.0 ** -10, 1.0),
        ("no faces", tetra, np.zeros((0, 3), I), np.array([0, 0, 1, 1], I),
         np.array([[0.5, 0, 0], [0, 0.5, 0.5]], F), np.ones(3), 2.0 ** -10, 1.0),
        ("no output", tetra, tetra_faces, np.full(4, -1, I), np.zeros((0, 3), F), np.ones(3),
         2.0 ** -10, 1.0),
        ("garbage",) + garbage_case() + (2.0 ** -10, 1.0),
    ]
    return cases


def _array(ctype, name, values):
    values = [int(x) for x in np.asarray(values).reshape(-1)]
    suffix = {"uint32_t": "u", "int32_t": "", "int64_t": "ll"}[ctype]
    body = ", ".join("%d%s" % (x, suffix) if x != -2 ** 31 else "(-2147483647 - 1)"
                     for x in values) or "0"
    return "static const %s %s[] = {%s};\n" % (ctype, name, body)


def expected_header(cases):
    """The cases and what the truth gives for them, as the C++ the host program includes: data
    only."""
    text = ["#pragma once\n#include <cstdint>\n",
            "struct Case {\n    const char *name;\n    int64_t nv, nf, nvo;\n"
            "    const uint32_t *vertices;\n    const int32_t *faces, *cluster;\n"
            "    const uint32_t *positions;\n    double cell[3], regularization, max_move;\n"
            "    const int64_t *sums;\n    const uint32_t *expected;\n    int64_t counts[2];\n};\n"]
    rows = []
    for i, (name, v, f, c, m, cell, reg, move) in enumerate(cases):
        S = qt.sums(v, f, c, m, cell)
        out, counts, _ = qt.solve(S, m, cell, reg, move)
        plain = qt.place_plain(v, f, c, m, cell, reg, move)
        assert np.array_equal(plain[2], S) and np.array_equal(qt.bits(plain[0]), qt.bits(out))
        text += [_array("uint32_t", "V%d" % i, qt.bits(v)), _array("int32_t", "F%d" % i, f),
                 _array("int32_t", "C%d" % i, c), _array("uint32_t", "M%d" % i, qt.bits(m)),
                 _array("int64_t", "S%d" % i, S), _array("uint32_t", "X%d" % i, qt.bits(out))]
        rows.append('    {"%s", %d, %d, %d, V%d, F%d, C%d, M%d, {%s, %s, %s}, %s, %s, S%d, X%d, '
                    '{%dll, %dll}},\n'
                    % (name, len(v), len(f), len(m), i, i, i, i, float(cell[0]).hex(),
                       float(cell[1]).hex(), float(cell[2]).hex(), float(reg).hex(),
                       float(move).hex(), i, i, counts[0], counts[1]))
    text += ["static const Case CASES[] = {\n"] + rows + ["};\n",
             "static const int N_CASES = %d;\n" % len(cases)]
    return "".join(text)


def test_checks_layout_and_phases_under_sanitizers(tmp_path):
    cases = host_cases()
    # the cases do what they are there for
    by_name = {c[0]: c for c in cases}
    S = qt.sums(*by_name["garbage"][1:6])
    out, counts, placed = qt.solve(S, by_name["garbage"][4], by_name["garbage"][5])
    assert placed.any() and not placed.all() and counts[1] > 0
    far = np.flatnonzero(by_name["garbage"][4][:, 0] > 30.0)    # the far position: nothing added
    assert len(far) == 1 and (S[far[0], :10] == 0).all() and S[far[0], 10] > 1
    assert S[0, 9] >= 2 ** 30                                   # the huge triangle weighs 1
    cube = by_name["cube"]
    assert qt.place(*cube[1:])[1][0] > 30
    with open(str(tmp_path / "quadric_expected.h"), "w") as f:
        f.write(expected_header(cases))
    printed = run_host_program("quadric", tmp_path, extra=("-I", str(tmp_path),
                                                            "-I", os.path.join(REPO, "tests")))
    assert "%d placements" % len(cases) in printed


def test_the_launcher_and_the_kernels_use_the_header():
    """raynet_quadric.inl decides on the header's verdict and lays the workspace out with its
    functions; the four kernels call one function of the header each in a grid-stride loop and add
    the index of the thread and the atomics policy: no subscript, no arithmetic on positions, no
    LDS, no floating-point atomic, no inline assembly; the header holds no HIP and no
    conditional."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_quadric.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "__syncthreads" not in code
    assert "while" not in code and "goto" not in code and "__shfl" not in code
    assert code.count("rn_qd::place_args(") == 1
    assert "if (verdict == rn_qd::INVALID)" in code and "if (verdict == rn_qd::EMPTY) return RN_OK;" in code
    for use in ("rn_qd::workspace_bytes(", "rn_qd::tables_of(", "rn_qd::solve_of(", "rn_qd::blocks("):
        assert use in code, use
    kernels = re.findall(r"__global__ __launch_bounds__\(BLOCK\) void (\w+)\(QuadricArgs a\) \{\n(.*?)\n\}\n",
                         code, re.S)
    calls = {"k_quadric_clear": "rn_qd::clear(", "k_quadric_members": "rn_qd::count_member(",
             "k_quadric_faces": "rn_qd::add_face(", "k_quadric_solve": "rn_qd::solve_vertex("}
    assert [k for k, _ in kernels] == list(calls)
    for name, body in kernels:
        assert body.count(calls[name]) == 1, name
        assert "[" not in body and "double" not in body and "float" not in body, name
        assert body.count("for (") == 1 and "+= stride" in body and "atomic" not in body, name
    assert re.findall(r"\batomic\w+", code) == ["atomicAdd"]
    assert "(unsigned long long *)p" in code                    # the one atomic is a 64-bit integer's
    header = open(os.path.join(CSRC, "raynet_quadric_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "while" not in hcode and "atomic" not in hcode
    assert "#pragma once" in header and '#include "raynet_mesh_args.h"' in header
    assert "rn_mesh::sizes_ok" in hcode and "rn_mesh::vertex_in" in hcode
    for f in ("raynet_quadric.inl", "raynet_quadric_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
    unit = open(os.path.join(CSRC, "raynet_hip.hip")).read()
    assert unit.count('#include "raynet_quadric.inl"') == 1
    assert unit.index('#include "raynet_simplify.inl"') < unit.index('#include "raynet_quadric.inl"')
    for f in ("raynet_quadric.inl", "raynet_quadric_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_entries_are_declared_and_bound_with_matching_types():
    """(The types of every entry, these included, and the restype of the size entry:
    tests/test_abi.py.)"""
    from raynet_amd import _lib
    want = {
        "rn_mesh_place_quadric_workspace_bytes": ("int64_t", ["int64_t nv", "int64_t nf",
                                                              "int64_t nvo"]),
        "rn_mesh_place_quadric": ("int", [
            "rn_ctx *ctx", "int64_t nv", "const float *vertices_in", "int64_t nf",
            "const int32_t *faces_in", "const int32_t *cluster", "int64_t nvo",
            "const float *positions_in", "const double cell[3]", "double regularization",
            "double max_move", "float *positions_out", "int64_t *counts", "void *workspace",
            "void *stream"])}
    lib = ctypes.CDLL(_lib.build())
    for name, prototype in want.items():
        assert abi_header.prototype(name) == prototype
        assert hasattr(lib, name)
    # the size entry needs no context and no GPU: the header's arithmetic
    fn = lib.rn_mesh_place_quadric_workspace_bytes
    fn.restype = ctypes.c_int64
    fn.argtypes = _lib.SIGNATURES["rn_mesh_place_quadric_workspace_bytes"]
    assert fn(0, 0, 0) == 0 and fn(257, 255, 100) == 8800 and fn(5, 0, 5) == 440
    assert fn(-1, 0, 0) == -1 and fn(5, -1, 0) == -1 and fn(5, 3, 6) == -1 and fn(5, 3, -1) == -1
    assert fn(2 ** 31 - 1, 0, 0) == -1 and fn(1, 2 ** 40, 0) == -1
    assert fn(2 ** 31 - 2, (2 ** 31 - 1) // 3, 2 ** 31 - 2) == 88 * (2 ** 31 - 2)


# ------------------------------------------------------------- the plumbing, on the truths' results
@pytest.fixture
def truth_calls(monkeypatch):
    """raynet_amd.simplify.mesh_simplify and mesh_place_quadric answered by the truths, and the
    vertex normals by theirs: the plumbing without a GPU."""
    import appearance_truth as at
    from raynet_amd import appearance, simplify
    calls = []

    def fake(vertices, faces, origin, cell, dims):
        calls.append(dict(what="simplify", cell=np.array(cell), origin=np.array(origin),
                          dims=np.array(dims)))
        return sp.simplify(vertices, faces, origin, cell, dims)

    def fake_place(vertices, faces, cluster, positions, cell, regularization, max_move):
        calls.append(dict(what="place", nv=len(vertices), nf=len(faces), nvo=len(positions),
                          cell=np.array(cell), regularization=regularization, max_move=max_move,
                          cluster=np.array(cluster), positions=np.array(positions)))
        return qt.place(vertices, faces, cluster, positions, cell, regularization, max_move)

    def fake_normals(vertices, faces, unit=True):
        calls.append(dict(what="normals"))
        n = at.area_normals(vertices, faces)
        return appearance.normalized(n) if unit else n

    monkeypatch.setattr(simplify, "mesh_simplify", fake)
    monkeypatch.setattr(simplify, "mesh_place_quadric", fake_place)
    monkeypatch.setattr(appearance, "vertex_normals", fake_normals)
    return calls


def _whats(calls):
    return [c["what"] for c in calls]


def test_simplify_mesh_places_by_quadrics_after_the_clustering(truth_calls):
    from raynet_amd.simplify import simplify_mesh
    vertices, faces = qt.rotated_cube(6)
    grid = sp.grid_around(vertices, 0.4)
    mean = sp.simplify(vertices, faces, *grid)
    want, counts = qt.place(vertices, faces, mean[3], mean[0], grid[1])
    # "mean" is today's path: one call, today's three values
    got = simplify_mesh(vertices, faces, 0.4)
    assert _whats(truth_calls) == ["simplify"] and len(got) == 3
    assert np.array_equal(qt.bits(got[0]), qt.bits(mean[0]))
    assert np.array_equal(qt.bits(simplify_mesh(vertices, faces, 0.4, placement="mean")[0]),
                          qt.bits(mean[0]))
    assert _whats(truth_calls) == ["simplify", "simplify"]
    del truth_calls[:]
    out, out_faces, source = simplify_mesh(vertices, faces, 0.4, placement="quadric")
    assert _whats(truth_calls) == ["simplify", "place"]
    call = truth_calls[-1]
    assert (call["nv"], call["nf"], call["nvo"]) == (218, 432, 48)
    assert np.array_equal(call["cell"], grid[1]) and np.array_equal(call["cluster"], mean[3])
    assert np.array_equal(qt.bits(call["positions"]), qt.bits(mean[0]))
    assert call["regularization"] == 2.0 ** -10 and call["max_move"] == 1.0
    assert np.array_equal(qt.bits(out), qt.bits(want)) and out.dtype == F
    assert np.array_equal(out_faces, sp.unique_faces(mean[1])[0]) and np.array_equal(source, mean[2])
    # the keywords reach the call, behind the old ones; the statistics are the entry's
    got = simplify_mesh(vertices, faces, (0.4, 0.5, 0.4), None, False, "quadric", 0.25, 0.05, True)
    call = truth_calls[-1]
    assert (call["regularization"], call["max_move"]) == (0.25, 0.05)
    assert np.array_equal(call["cell"], [0.4, 0.5, 0.4])
    grid2 = sp.grid_around(vertices, (0.4, 0.5, 0.4))
    mean2 = sp.simplify(vertices, faces, *grid2)
    want2, counts2 = qt.place(vertices, faces, mean2[3], mean2[0], grid2[1], 0.25, 0.05)
    assert np.array_equal(qt.bits(got[0]), qt.bits(want2)) and np.array_equal(got[1], mean2[1])
    moved = np.abs(want2.astype(D) - mean2[0].astype(D)) / grid2[1]
    assert got[3] == {"moved": int(counts2[0]), "fell_back": int(counts2[1]),
                      "farthest_move": float(moved.max())}
    assert 0.04 < got[3]["farthest_move"] < 0.0501
    assert simplify_mesh(vertices, faces, 0.4, return_stats=True)[3] == \
        {"moved": 0, "fell_back": 0, "farthest_move": 0.0}
    # everything in one cell: no output vertex, no second call
    del truth_calls[:]
    gone = simplify_mesh(vertices, faces, 100.0, origin=(-50.0, -50.0, -50.0), placement="quadric")
    assert len(gone[0]) == 0 and _whats(truth_calls) == ["simplify"]
    # the refusals name the argument, and nothing reaches a GPU call
    del truth_calls[:]
    nan, inf = float("nan"), float("inf")
    for kw, match in [(dict(placement="median"), "placement"), (dict(placement=None), "placement"),
                      (dict(regularization=0.0), "regularization"),
                      (dict(regularization=2.0 ** -21), "regularization"),
                      (dict(regularization=1.5), "regularization"),
                      (dict(regularization=nan), "regularization"),
                      (dict(regularization="x"), "regularization"),
                      (dict(max_move=0.0), "max_move"), (dict(max_move=-1.0), "max_move"),
                      (dict(max_move=nan), "max_move"), (dict(max_move=None), "max_move"),
                      (dict(placement="mean", regularization=7.0), "regularization")]:
        args = dict(vertices=vertices, faces=faces, cell=0.4, placement="quadric")
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            simplify_mesh(**args)
    assert truth_calls == []
    assert len(simplify_mesh(vertices, faces, 0.4, placement="quadric", max_move=inf,
                             regularization=2.0 ** -20)[0]) == 48


def test_surface_mesh_simplified_takes_the_three_keywords(truth_calls):
    import appearance_truth as at
    from raynet_amd import appearance
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = qt.rotated_cube(6)
    rng = np.random.default_rng(2)
    colors = rng.integers(0, 256, size=vertices.shape).astype(np.uint8)
    grid = sp.grid_around(vertices, 0.4)
    mean = sp.simplify(vertices, faces, *grid)
    want, counts = qt.place(vertices, faces, mean[3], mean[0], grid[1])
    want_faces = sp.unique_faces(mean[1])[0]
    mesh = SurfaceMesh(vertices, faces, vertices.copy(), colors)
    parameters = list(inspect.signature(SurfaceMesh.simplified).parameters)
    assert parameters[:7] == ["self", "cell", "origin", "drop_duplicate_faces", "placement",
                              "regularization", "max_move"]
    plain = mesh.simplified(0.4)
    assert _whats(truth_calls) == ["simplify", "normals"]
    assert np.array_equal(qt.bits(plain.vertices), qt.bits(mean[0]))
    del truth_calls[:]
    out = mesh.simplified(0.4, placement="quadric")
    assert _whats(truth_calls) == ["simplify", "place", "normals"]
    assert np.array_equal(qt.bits(out.vertices), qt.bits(want)) and np.array_equal(out.faces, want_faces)
    assert np.array_equal(out.colors, colors[mean[2]])          # colours stay those of `source`
    assert np.array_equal(qt.bits(out.normals),                 # normals are of the placed vertices
                          qt.bits(appearance.normalized(at.area_normals(want, want_faces))))
    assert np.array_equal(qt.bits(mesh.vertices), qt.bits(vertices))
    held, stats = mesh.simplified(0.4, None, True, "quadric", 1.0, 0.5, return_stats=True)
    assert (truth_calls[-2]["regularization"], truth_calls[-2]["max_move"]) == (1.0, 0.5)
    assert stats["moved"] > 30 and stats["fell_back"] == 0 and 0 < stats["farthest_move"] <= 0.5
    bare = SurfaceMesh(vertices, faces).simplified(0.4, placement="quadric")
    assert bare.normals is None and bare.colors is None
    with pytest.raises(ValueError, match="placement"):
        mesh.simplified(0.4, placement="best")
    # an empty mesh: checked, not computed
    del truth_calls[:]
    empty = SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), I))
    assert empty.simplified(1.0, placement="quadric").empty
    with pytest.raises(ValueError, match="regularization"):
        empty.simplified(1.0, placement="quadric", regularization=2.0)
    assert truth_calls == []


# ------------------------------------------------------------------------------ the scripts
def test_the_flag_helper_places_and_reports(truth_calls, capsys):
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    from raynet_amd.volume import SurfaceMesh
    assert mesh_flags.PLACEMENT_FLAGS == ("simplify_placement", "simplify_regularization")
    assert not set(mesh_flags.PLACEMENT_FLAGS) & set(mesh_flags.FLAGS)
    vertices, faces = qt.rotated_cube(6)
    mesh = SurfaceMesh(vertices, faces)
    voxel, corner = np.array([0.2, 0.2, 0.2]), np.array([-1.0, -1.0, -1.0])
    parser = fuse_depth_maps.build_parser()
    # without the new flags: the line of today, one call
    args = parser.parse_args(["s", "p", "o.ply", "--simplify", "2"])
    assert args.simplify_placement is None and args.simplify_regularization is None
    assert mesh_flags.given(args, mesh_flags.PLACEMENT_FLAGS) == []
    plain = mesh_flags.simplify(mesh, args, voxel, corner)
    printed = capsys.readouterr().out
    assert printed.startswith("simplify: cell 2 voxel sides, 218 -> ") and printed.count("\n") == 1
    assert "placement" not in printed and _whats(truth_calls) == ["simplify"]
    # --simplify_placement mean: the same
    args = parser.parse_args(["s", "p", "o.ply", "--simplify", "2", "--simplify_placement", "mean"])
    same = mesh_flags.simplify(mesh, args, voxel, corner)
    assert capsys.readouterr().out == printed and _whats(truth_calls) == ["simplify"] * 2
    assert np.array_equal(qt.bits(same.vertices), qt.bits(plain.vertices))
    # quadric: the second line, from the arrays
    del truth_calls[:]
    args = parser.parse_args(["s", "p", "o.ply", "--simplify", "2", "--simplify_placement", "quadric"])
    assert mesh_flags.given(args, mesh_flags.PLACEMENT_FLAGS) == ["simplify_placement"]
    out = mesh_flags.simplify(mesh, args, voxel, corner)
    assert _whats(truth_calls) == ["simplify", "place"]
    call = truth_calls[0]
    assert np.array_equal(call["cell"], 2.0 * voxel) and truth_calls[1]["regularization"] == 2.0 ** -10
    mean = sp.simplify(vertices, faces, call["origin"], call["cell"], call["dims"])
    want, counts = qt.place(vertices, faces, mean[3], mean[0], call["cell"])
    assert np.array_equal(qt.bits(out.vertices), qt.bits(want)) and np.array_equal(out.faces, plain.faces)
    moved = (np.abs(want.astype(D) - mean[0].astype(D)) / call["cell"]).max()
    lines = capsys.readouterr().out.splitlines()
    assert lines == [printed.strip(),
                     "placement: quadric, %d of %d vertices moved, %d fell back, farthest move "
                     "%.3f cell sides" % (counts[0], len(want), counts[1], moved)]
    assert counts[0] == (qt.bits(want) != qt.bits(mean[0])).any(1).sum() > 0
    args = parser.parse_args(["s", "p", "o.ply", "--simplify", "2", "--simplify_placement", "quadric",
                              "--simplify_regularization", "0.5"])
    assert mesh_flags.given(args, mesh_flags.PLACEMENT_FLAGS) == list(mesh_flags.PLACEMENT_FLAGS)
    mesh_flags.simplify(mesh, args, voxel, corner)
    assert truth_calls[-1]["regularization"] == 0.5


def test_the_scripts_know_the_flags_and_refuse_bad_values(tmp_path, capsys):
    from raynet_amd.scripts import fuse_depth_maps, render_volume
    out = str(tmp_path / "out.ply")
    occupancy = str(tmp_path / "occupancy.npz")
    np.savez(open(occupancy, "wb"), belief=np.zeros((2, 2, 2), F), bbox=np.zeros(6, F),
             grid_shape=np.array([2, 2, 2], I))
    cases = [(fuse_depth_maps, ["scene", "predictions", out], []),
             (render_volume, ["scene", occupancy, str(tmp_path / "maps")], ["--mesh", out])]
    for script, positional, mesh_flag in cases:
        a = script.build_parser().parse_args(positional + ["--simplify", "2", "--simplify_placement",
                                                           "quadric", "--simplify_regularization",
                                                           "0.125"])
        assert (a.simplify_placement, a.simplify_regularization) == ("quadric", 0.125)
        quadric = ["--simplify", "2", "--simplify_placement", "quadric"]
        for argv, message in [
                (["--simplify_placement", "quadric"], "--simplify_placement"),
                (["--simplify_placement", "mean"], "--simplify_placement"),
                (["--simplify", "2", "--simplify_placement", "median"], "--simplify_placement"),
                (["--simplify_regularization", "0.5"], "--simplify_regularization"),
                (["--simplify", "2", "--simplify_regularization", "0.5"], "--simplify_regularization"),
                (["--simplify", "2", "--simplify_placement", "mean", "--simplify_regularization",
                  "0.5"], "--simplify_regularization"),
                (quadric + ["--simplify_regularization", "0"], "--simplify_regularization"),
                (quadric + ["--simplify_regularization", "1e-7"], "--simplify_regularization"),
                (quadric + ["--simplify_regularization", "1.5"], "--simplify_regularization"),
                (quadric + ["--simplify_regularization", "nan"], "--simplify_regularization")]:
            with pytest.raises(SystemExit) as e:
                script.main(positional + mesh_flag + argv)
            assert e.value.code == 2
            assert message in capsys.readouterr().err, (script.__name__, argv)
    # render_volume: the flags are the mesh's
    with pytest.raises(SystemExit) as e:
        render_volume.main(cases[1][1] + ["--simplify", "2", "--simplify_placement", "quadric"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--simplify" in err and "--mesh" in err
    assert not os.path.exists(out)
    # the flags of today are what they were, and the new ones are registered behind them
    from raynet_amd.scripts import mesh_flags
    assert mesh_flags.FLAGS == (mesh_flags.COMPONENT_FLAGS + mesh_flags.SIMPLIFY_FLAGS +
                                mesh_flags.SMOOTH_FLAGS)
    source = inspect.getsource(mesh_flags.add_arguments)
    assert source.index("--fill_holes") < source.index("--simplify_placement") < \
        source.index("--simplify_regularization")
