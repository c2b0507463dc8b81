"""Taubin smoothing, the host side (no GPU): the argument checks, the workspace layout, the ring and
the step of the kernels (raynet_amd/csrc/raynet_smooth_args.h) as a stand-alone program under the
address and undefined-behaviour sanitizers -- nothing sanitised is loaded into this interpreter --
the kernels' use of that header, the entries in the header and the ctypes table, smooth_vertices
and SurfaceMesh.smoothed against tests/smooth_truth.py with the truth in place of the GPU call,
boundary_vertices by the torch route on the CPU device, and the flags of the two mesh-writing
scripts."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_header
import components_truth as ct
import smooth_truth as st
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_checks_ring_and_steps_under_sanitizers(tmp_path):
    run_host_program("smooth", tmp_path)


def test_the_launcher_and_the_kernels_use_the_header():
    """raynet_smooth.inl decides on the header's verdict, lays out the workspace and walks the
    steps with its functions; the kernels call ring_entry / step_vertex and add the index of the
    thread: no subscript, no arithmetic on positions, no atomics, no LDS; the header holds no HIP."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_smooth.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "__syncthreads" not in code
    assert "atomic" not in code and "while" not in code and "goto" not in code
    assert code.count("rn_sm::smooth_args(") == 1
    assert "if (verdict == rn_sm::INVALID)" in code and "if (verdict == rn_sm::EMPTY) return RN_OK;" in code
    for use in ("rn_sm::step_count(", "rn_sm::step_factor(", "rn_sm::step_source(",
                "rn_sm::step_target(", "rn_sm::scratch_offset(", "rn_sm::workspace_bytes(",
                "rn_sm::sizes_ok(", "rn_sm::blocks("):
        assert use in code, use
    kernels = re.findall(r"__global__ __launch_bounds__\(BLOCK\) void (\w+)\(SmoothArgs a\) \{\n(.*?)\n\}\n",
                         code, re.S)
    assert [k for k, _ in kernels] == ["k_smooth_ring", "k_smooth_step"]
    for (name, body), call, guard in zip(kernels, ("rn_sm::ring_entry(", "rn_sm::step_vertex("),
                                         ("rn_sm::corner_in(k, a.nf)", "rn_sm::vertex_in(v, a.nv)")):
        assert body.count(call) == 1 and guard in body, name
        assert "[" not in body and "double" not in body and "float" not in body, name
        assert body.count("for (") == 1 and "+= stride" in body, name
    header = open(os.path.join(CSRC, "raynet_smooth_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "while" not in hcode
    for f in ("raynet_smooth.inl", "raynet_smooth_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
    assert '#include "raynet_smooth.inl"' in open(os.path.join(CSRC, "raynet_hip.hip")).read()
    for f in ("raynet_smooth.inl", "raynet_smooth_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_entries_are_declared_and_bound_with_matching_types():
    """(The types of every entry, these included, and the restype of the size entry:
    tests/test_abi.py.)"""
    from raynet_amd import _lib
    want = {
        "rn_mesh_smooth_workspace_bytes": ("int64_t", ["rn_ctx *ctx", "int64_t nv", "int64_t nf"]),
        "rn_mesh_smooth": ("int", [
            "rn_ctx *ctx", "int64_t nv", "const float *vertices_in", "int64_t nf",
            "const int32_t *faces", "const int32_t *offsets", "const int32_t *corners",
            "const uint8_t *fixed", "int32_t iterations", "double lambda", "double mu",
            "double max_move", "void *workspace", "float *vertices_out", "void *stream"])}
    lib = ctypes.CDLL(_lib.build())
    for name, prototype in want.items():
        assert abi_header.prototype(name) == prototype
        assert hasattr(lib, name)


# ------------------------------------------------------------- the plumbing, on the truth's steps
@pytest.fixture
def truth_steps(monkeypatch):
    """raynet_amd.smoothing.mesh_smooth answered by the truth, and the vertex normals by theirs:
    the plumbing without a GPU."""
    import appearance_truth as at
    from raynet_amd import appearance, smoothing
    calls = []

    def fake(vertices, faces, fixed, iterations, lam, mu, max_move):
        calls.append(dict(nv=len(vertices), nf=len(faces), iterations=iterations, lam=lam, mu=mu,
                          max_move=max_move, fixed=None if fixed is None else np.array(fixed)))
        return st.smooth(vertices, faces, iterations, lam, mu, fixed, max_move)

    def fake_normals(vertices, faces, unit=True):
        calls.append("normals")
        n = at.area_normals(vertices, faces)
        return appearance.normalized(n) if unit else n

    monkeypatch.setattr(smoothing, "mesh_smooth", fake)
    monkeypatch.setattr(appearance, "vertex_normals", fake_normals)
    return calls


def _open_mesh(seed=0):
    """A flat patch shaken out of its plane, ids permuted and faces shuffled, two loose vertices."""
    vertices, faces = st.flat_patch(7)
    nv = len(vertices)
    rng = np.random.default_rng(seed)
    vertices = vertices + rng.normal(scale=0.1, size=vertices.shape).astype(F)
    faces, order = ct.shuffled(faces, nv, seed)
    moved = np.empty_like(vertices)
    moved[order] = vertices
    return np.concatenate([moved, st.positions(2, seed)]), faces


def test_smooth_vertices_is_the_truth_and_pins_what_it_is_told(truth_steps):
    from raynet_amd.smoothing import smooth_vertices
    vertices, faces = _open_mesh()
    nv = len(vertices)
    border = st.boundary_vertices(faces, nv)
    assert 0 < border.sum() < nv - 2
    out = smooth_vertices(vertices, faces)
    assert out.dtype == F and out.shape == (nv, 3)
    call = truth_steps[-1]
    assert (call["iterations"], call["lam"], call["mu"], call["max_move"]) == (10, 0.5, -0.53, np.inf)
    assert np.array_equal(call["fixed"] != 0, border)
    assert np.array_equal(_bits(out), _bits(st.smooth(vertices, faces, 10, 0.5, -0.53, border)))
    assert np.array_equal(_bits(out[border]), _bits(vertices[border]))
    # nothing pinned, a mask, lists and tensors
    import torch
    free = smooth_vertices(torch.from_numpy(vertices), faces.tolist(), 3, fixed=None, max_move=0.05)
    assert truth_steps[-1]["fixed"] is None and truth_steps[-1]["max_move"] == 0.05
    assert np.array_equal(_bits(free), _bits(st.smooth(vertices, faces, 3, max_move=0.05)))
    assert not np.array_equal(free[border], vertices[border])
    mask = np.zeros(nv, np.uint8)
    mask[::3] = 7
    some = smooth_vertices(vertices, faces, 2, 0.6, 0.0, fixed=mask)
    assert np.array_equal(_bits(some), _bits(st.smooth(vertices, faces, 2, 0.6, 0.0, mask)))
    assert np.array_equal(_bits(some[::3]), _bits(vertices[::3]))
    # the refusals name the argument, and nothing reaches the GPU call
    n = len(truth_steps)
    for kw, match in [(dict(iterations=-1), "iterations"), (dict(iterations=10001), "iterations"),
                      (dict(iterations=2.5), "iterations"),
                      (dict(lam=0.0), "lam"), (dict(lam=1.5), "lam"), (dict(lam=float("nan")), "lam"),
                      (dict(mu=0.1), "mu"), (dict(mu=-1.5), "mu"), (dict(mu=float("-inf")), "mu"),
                      (dict(max_move=0.0), "max_move"), (dict(max_move=-1.0), "max_move"),
                      (dict(max_move=float("nan")), "max_move"),
                      (dict(fixed=np.zeros(nv - 1, bool)), "fixed"), (dict(fixed="border"), "fixed"),
                      (dict(faces=np.array([[0, 1, nv]])), "faces"),
                      (dict(faces=np.array([[0, -1, 2]])), "faces")]:
        args = dict(vertices=vertices, faces=faces)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            smooth_vertices(**args)
    assert len(truth_steps) == n
    # the limits themselves are taken; no vertices: nothing to do
    smooth_vertices(vertices, faces, 0, lam=1.0, mu=-1.0, max_move=float("inf"))
    assert smooth_vertices(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)).shape == (0, 3)
    assert len(truth_steps) == n + 1


def test_surface_mesh_smoothed_carries_colours_and_recomputes_normals_only_if_present(truth_steps):
    import appearance_truth as at
    from raynet_amd import appearance
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = _open_mesh(1)
    nv = len(vertices)
    rng = np.random.default_rng(1)
    colors = rng.integers(0, 256, size=(nv, 3)).astype(np.uint8)
    stale = rng.normal(size=(nv, 3)).astype(F)
    want = st.smooth(vertices, faces, 4, 0.5, -0.53, st.boundary_vertices(faces, nv), 0.3)
    # bare
    mesh = SurfaceMesh(vertices, faces)
    out = mesh.smoothed(iterations=4, max_move=0.3)
    assert out is not mesh and np.array_equal(_bits(out.vertices), _bits(want))
    assert np.array_equal(out.faces, faces) and out.faces is not mesh.faces
    assert out.normals is None and out.colors is None and "normals" not in truth_steps
    assert np.array_equal(_bits(mesh.vertices), _bits(vertices))            # the mesh itself stays
    # colours alone go along, and no normals appear
    out = SurfaceMesh(vertices, faces, colors=colors).smoothed(iterations=4, max_move=0.3)
    assert np.array_equal(out.colors, colors) and out.normals is None and "normals" not in truth_steps
    # normals: recomputed from the new positions
    mesh = SurfaceMesh(vertices, faces, stale, colors)
    out = mesh.smoothed(iterations=4, max_move=0.3)
    assert truth_steps[-1] == "normals"
    assert np.array_equal(_bits(out.normals), _bits(appearance.normalized(at.area_normals(want, faces))))
    assert np.array_equal(out.colors, colors) and np.array_equal(_bits(mesh.normals), _bits(stale))
    # the keywords are smooth_vertices' own
    out = mesh.smoothed(2, 0.4, 0.0, None, None)
    assert np.array_equal(_bits(out.vertices), _bits(st.smooth(vertices, faces, 2, 0.4, 0.0)))
    with pytest.raises(ValueError, match="mu"):
        mesh.smoothed(mu=0.5)


def test_an_empty_mesh_stays_empty_without_the_gpu(truth_steps):
    from raynet_amd.volume import SurfaceMesh
    loose = st.positions(4, 2)
    for mesh in (SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)),
                 SurfaceMesh(loose, np.zeros((0, 3), np.int32), loose, np.zeros((4, 3), np.uint8))):
        out = mesh.smoothed()
        assert out is not mesh and out.empty and out.faces.shape == (0, 3)
        assert np.array_equal(_bits(out.vertices), _bits(mesh.vertices))
        assert (out.normals is None) == (mesh.normals is None)
        assert (out.colors is None) == (mesh.colors is None)
        with pytest.raises(ValueError, match="lam"):
            mesh.smoothed(lam=0.0)
    assert truth_steps == []                         # nobody asked the GPU, or for normals


def test_boundary_vertices_by_the_torch_route_is_the_truths():
    import torch
    from raynet_amd.smoothing import boundary_vertices
    cases = [_open_mesh(3)[1:] + (51,), (ct.strip(40), 40), ct.tetrahedra(5), ct.star(9),
             (ct.tetrahedra(3)[0][1:], 12), (np.zeros((0, 3), np.int32), 4),
             (np.zeros((0, 3), np.int32), 0),
             (np.array([[1, 1, 3], [0, 2, 4], [2, 0, 9], [-1, 2, 3]], np.int32), 5)]
    vertices, faces = st.binary_ball()
    cases.append((faces, len(vertices)))
    cases.append((faces[::2], len(vertices)))
    for faces, nv in cases:
        if len(faces) > 3:
            faces, _ = ct.shuffled(faces, nv, seed=nv)
        want = st.boundary_vertices(faces, nv)
        got = boundary_vertices(torch.from_numpy(np.ascontiguousarray(faces, np.int32)), nv)
        assert got.dtype == torch.bool and got.device.type == "cpu" and tuple(got.shape) == (nv,)
        assert np.array_equal(got.numpy(), want), nv
        assert np.array_equal(boundary_vertices(np.asarray(faces, np.int64), nv).numpy(), want)
    assert not st.boundary_vertices(cases[-2][0], cases[-2][1]).any()      # the ball is closed
    assert st.boundary_vertices(cases[-1][0], cases[-1][1]).any()


# ------------------------------------------------------------------------------ the scripts
def test_the_flag_helper_smooths_and_reports(truth_steps, capsys, tmp_path):
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = _open_mesh(4)
    mesh = SurfaceMesh(vertices, faces)
    voxel = np.array([0.5, 0.25, 1.0])
    # without --smooth: the very object, nothing printed, and so the bytes of the file
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply"])
    assert mesh_flags.given(args) == []
    assert mesh_flags.smooth(mesh, args, voxel) is mesh and capsys.readouterr().out == ""
    assert truth_steps == []
    before, after = str(tmp_path / "before.ply"), str(tmp_path / "after.ply")
    mesh.save_ply(before)
    mesh_flags.smooth(mesh, args, voxel).save_ply(after)
    assert open(before, "rb").read() == open(after, "rb").read()
    # --smooth 3: the defaults -- lambda 0.5, mu -0.53, one side of the smallest voxel, border pinned
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--smooth", "3"])
    out = mesh_flags.smooth(mesh, args, voxel)
    border = st.boundary_vertices(faces, len(vertices))
    want = st.smooth(vertices, faces, 3, 0.5, -0.53, border, 0.25)
    assert np.array_equal(_bits(out.vertices), _bits(want))
    far = np.abs(want.astype(np.float64) - vertices.astype(np.float64)).max() / 0.25
    assert capsys.readouterr().out == \
        "smooth: 3 iterations, %d vertices, farthest move %.3f voxel sides\n" % (len(vertices), far)
    # every flag
    args = fuse_depth_maps.build_parser().parse_args([
        "s", "p", "o.ply", "--smooth", "2", "--smooth_lambda", "0.6", "--smooth_mu", "0",
        "--smooth_max_move", "inf", "--smooth_free_boundary"])
    out = mesh_flags.smooth(mesh, args, voxel)
    assert np.array_equal(_bits(out.vertices), _bits(st.smooth(vertices, faces, 2, 0.6, 0.0)))
    assert truth_steps[-1]["fixed"] is None and truth_steps[-1]["max_move"] == np.inf
    args = fuse_depth_maps.build_parser().parse_args([
        "s", "p", "o.ply", "--smooth", "2", "--smooth_max_move", "0.1"])
    out = mesh_flags.smooth(mesh, args, voxel)
    assert truth_steps[-1]["max_move"] == 0.1 * 0.25
    assert np.abs(out.vertices.astype(np.float64) - vertices).max() <= 0.025 + 1e-6


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
        assert a.smooth is None and a.smooth_lambda is None and a.smooth_mu is None
        assert a.smooth_max_move is None and not a.smooth_free_boundary
        a = script.build_parser().parse_args(positional + [
            "--smooth", "7", "--smooth_lambda", "0.4", "--smooth_mu", "-0.45",
            "--smooth_max_move", "2.5", "--smooth_free_boundary"])
        assert (a.smooth, a.smooth_lambda, a.smooth_mu, a.smooth_max_move,
                a.smooth_free_boundary) == (7, 0.4, -0.45, 2.5, True)
        for argv, message in [
                (["--smooth", "0"], "--smooth"), (["--smooth", "-2"], "--smooth"),
                (["--smooth", "10001"], "--smooth"),
                (["--smooth", "3", "--smooth_lambda", "0"], "--smooth_lambda"),
                (["--smooth", "3", "--smooth_lambda", "1.01"], "--smooth_lambda"),
                (["--smooth", "3", "--smooth_lambda", "nan"], "--smooth_lambda"),
                (["--smooth", "3", "--smooth_mu", "0.1"], "--smooth_mu"),
                (["--smooth", "3", "--smooth_mu", "-1.5"], "--smooth_mu"),
                (["--smooth", "3", "--smooth_mu", "-inf"], "--smooth_mu"),
                (["--smooth", "3", "--smooth_max_move", "0"], "--smooth_max_move"),
                (["--smooth", "3", "--smooth_max_move", "-1"], "--smooth_max_move"),
                (["--smooth", "3", "--smooth_max_move", "nan"], "--smooth_max_move"),
                (["--smooth_lambda", "0.5"], "--smooth_lambda"),
                (["--smooth_free_boundary"], "--smooth_free_boundary")]:
            with pytest.raises(SystemExit) as e:
                script.main(positional + mesh_flag + argv)
            assert e.value.code == 2
            assert message in capsys.readouterr().err, (script.__name__, argv)
    # render_volume: the flags are the mesh's
    for argv, message in [(["--smooth", "3"], "--smooth"),
                          (["--smooth", "3", "--smooth_mu", "-0.6", "--mesh_cloud", out,
                            "--mesh_samples", "10"], "--smooth")]:
        with pytest.raises(SystemExit) as e:
            render_volume.main(cases[1][1] + argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err and "--mesh" in err, argv
    assert not os.path.exists(out)
