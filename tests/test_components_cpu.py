"""Connected components, the host side (no GPU): the argument checks and the union-find of the
kernels (raynet_amd/csrc/raynet_components_args.h) as a stand-alone program under the address and
undefined-behaviour sanitizers and under the thread sanitizer -- nothing sanitised is loaded into
this interpreter -- the kernels' use of that header, the entry in the header and the ctypes table,
MeshComponents and the SurfaceMesh methods against tests/components_truth.py with the truth's
labels in place of the GPU's, and the flags of the two mesh-writing scripts."""
import ctypes
import os
import re

import numpy as np
import pytest

import components_truth as ct
import abi_header
from conftest import REPO
from host_program import run_host_program

F = np.float32
CSRC = os.path.join(REPO, "raynet_amd", "csrc")


@pytest.mark.parametrize("sanitizers", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                                        ["-fsanitize=thread"]], ids=["asan-ubsan", "tsan"])
def test_checks_and_union_find_under_sanitizers(tmp_path, sanitizers):
    run_host_program("components", tmp_path, sanitizers, extra=["-pthread"])


def _kernel(code, name):
    m = re.search(r"void %s\(ComponentsArgs a\) \{\n(.*?)\n\}\n" % name, code, re.S)
    assert m is not None, name
    return m.group(1)


def test_the_launcher_and_the_kernels_use_the_header():
    """raynet_components.inl decides on the header's verdict, unites and finds with its templates,
    and writes the parent array in k_cc_hook only through the policy's compare-and-swap; the
    policy is relaxed and at agent scope; the header holds no HIP."""
    from raynet_amd import _lib
    src = open(os.path.join(CSRC, "raynet_components.inl")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "__shared__" not in code and "__syncthreads" not in code
    assert "while" not in code and "goto" not in code
    assert code.count("rn_cc::components_args(") == 1
    assert "if (verdict == rn_cc::INVALID)" in code and "if (verdict == rn_cc::EMPTY) return RN_OK;" in code
    for use in ("rn_cc::unite(", "rn_cc::face_counts_in(", "rn_cc::face_index(", "rn_cc::blocks(",
                "rn_cc::step_bound(", "rn_cc::vertex_in("):
        assert use in code, use
    # the four kernels, one by-value argument struct each
    assert re.findall(r"__global__ __launch_bounds__\(BLOCK\) void (\w+)\(ComponentsArgs a\)", code) \
        == ["k_cc_init", "k_cc_hook", "k_cc_flatten", "k_cc_count"]
    # the policy: every access relaxed, at agent scope
    policy = re.search(r"struct AgentAtomics \{.*?\n\};", code, re.S).group(0)
    assert policy.count("__hip_atomic_load(") == 1
    assert policy.count("__hip_atomic_compare_exchange_strong(") == 1
    assert policy.count("__hip_atomic_store(") == 1
    assert policy.count("__HIP_MEMORY_SCOPE_AGENT") == 3 and "__ATOMIC_SEQ_CST" not in policy
    assert code.count("__hip_atomic_") == 3                  # nowhere else
    # k_cc_hook: the parent array only through the policy -- no subscript of labels, no plain store
    hook = _kernel(code, "k_cc_hook")
    assert hook.count("labels") == 1 and "const AgentAtomics at{a.labels};" in hook
    assert len(re.findall(r"\]\s*=(?!=)", hook)) == 1 and "a.status[0] = 1;" in hook
    assert not re.search(r"\*\s*\w+\s*=(?!=)", hook) and "atomic" not in hook
    # the header's unite / find write through `cas` only, and read through `load` only
    header = open(os.path.join(CSRC, "raynet_components_args.h")).read()
    hcode = re.sub(r"//.*", "", header)
    assert "hip" not in hcode.lower() and "parent" not in hcode
    assert hcode.count("at.cas(") == 2 and hcode.count("at.load(") == 4
    # the one store of the policy is flatten's, after the hooks' launch; unite and find have none
    assert hcode.count("at.store(") == 1
    flatten = hcode[hcode.index("constexpr bool flatten("):]
    assert "at.store(v, x);" in flatten and "at.cas(" not in flatten
    assert "while" not in hcode                               # every loop is a bounded for
    assert hcode.count("for (") == 3 and hcode.count("step >= bound") == 2 and "tries < bound" in hcode
    # k_cc_flatten runs the header's flatten; the only plain store to labels is init's
    assert "rn_cc::flatten(at, " in _kernel(code, "k_cc_flatten")
    assert len(re.findall(r"labels\[[^\]]*\]\s*=(?!=)", code)) == 1
    assert "a.labels[v] = (int32_t)v;" in _kernel(code, "k_cc_init")
    for f in ("raynet_components.inl", "raynet_components_args.h"):
        assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", open(os.path.join(CSRC, f)).read(),
                             re.M), f
    assert '#include "raynet_components.inl"' in open(os.path.join(CSRC, "raynet_hip.hip")).read()
    for f in ("raynet_components.inl", "raynet_components_args.h"):
        assert os.path.join(CSRC, f) in _lib.sources(), f


def test_the_entry_is_declared_and_bound_with_matching_types():
    """(The types of every entry, this one included: tests/test_abi.py.)"""
    from raynet_amd import _lib
    assert abi_header.prototype("rn_mesh_components") == ("int", [
        "rn_ctx *ctx", "int64_t nv", "int64_t nf", "const int32_t *faces", "int32_t *labels",
        "int32_t *vertex_counts", "int32_t *face_counts", "int32_t *status", "void *stream"])
    assert hasattr(ctypes.CDLL(_lib.build()), "rn_mesh_components")


# ------------------------------------------------------------- the plumbing, on the truth's labels
@pytest.fixture
def truth_labels(monkeypatch):
    """raynet_amd.components.mesh_components answered by the truth: the plumbing without a GPU."""
    from raynet_amd import components
    calls = []

    def fake(faces, n_vertices):
        calls.append((len(faces), int(n_vertices)))
        return components.MeshComponents(*ct.components(faces, int(n_vertices)))

    monkeypatch.setattr(components, "mesh_components", fake)
    return calls


def _pieces(seed=0):
    """Tetrahedra, triangles, a strip and a star in one mesh with shuffled ids and faces, and
    vertices in no face; random positions, normals and colours."""
    parts, at = [], 0
    for faces, nv in (ct.tetrahedra(7), ct.triangles(5), (ct.strip(40), 40), ct.star(23),
                      (np.zeros((0, 3), np.int32), 6), ct.tetrahedra(1), (ct.strip(12), 12)):
        parts.append(np.asarray(faces, np.int64) + at)
        at += nv
    faces, _ = ct.shuffled(np.concatenate(parts), at, seed)
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(at, 3)).astype(F), faces, rng.normal(size=(at, 3)).astype(F),
            rng.integers(0, 256, size=(at, 3)).astype(np.uint8))


def test_mesh_components_fields_are_the_truths():
    from raynet_amd.components import MeshComponents
    _, faces, _, _ = _pieces()
    nv = int(faces.max()) + 1 + 2
    labels, vc, fc = ct.components(faces, nv)
    c = MeshComponents(labels, vc, fc)
    roots, component, n_vertices, n_faces = ct.dense(labels, vc, fc)
    assert c.labels.dtype == np.int32 and np.array_equal(c.labels, labels)
    assert np.array_equal(c.roots, roots) and np.array_equal(c.component, component)
    assert np.array_equal(c.n_vertices, n_vertices) and np.array_equal(c.n_faces, n_faces)
    assert len(c) == len(roots) and (np.diff(c.roots) > 0).all()
    assert np.array_equal(c.roots[c.component], c.labels)
    assert np.array_equal(c.face_component(faces), component[faces[:, 0]])
    for k in (0, 1, 2, 5, len(roots), len(roots) + 3):
        assert np.array_equal(c.largest(k), ct.largest(n_faces, k)), k
    for kw in (dict(min_faces=1), dict(min_faces=4), dict(min_faces=5), dict(min_faces=10 ** 6),
               dict(min_fraction=1.0), dict(min_fraction=0.5), dict(min_fraction=4 / 38),
               dict(min_fraction=1e-9), dict(keep_largest=1), dict(keep_largest=3),
               dict(keep_largest=10 ** 6), dict(min_faces=4, keep_largest=9),
               dict(min_faces=2, min_fraction=0.2, keep_largest=2), dict()):
        got = c.select(**kw)
        assert got.dtype == bool and np.array_equal(got, ct.select(n_faces, **kw)), kw
        assert not got[n_faces == 0].any()
    # faces that name no vertex belong to no component and are never kept
    planted, hit = ct.with_garbage(faces, nv, seed=3, fraction=0.2)
    g = MeshComponents(*ct.components(planted, nv))
    of = g.face_component(planted)
    assert hit.any() and (of[hit] == -1).all() and (of[~hit] >= 0).all()
    assert np.array_equal(of[~hit], g.component[planted[~hit, 0]])
    assert np.array_equal(g.face_mask(planted, np.ones(len(g), bool)), ~hit)
    assert not g.face_mask(planted, np.zeros(len(g), bool)).any()
    # ties go to the lower id
    tied = MeshComponents(*ct.components(*ct.tetrahedra(5)))
    assert tied.largest(2).tolist() == [0, 1] and tied.select(keep_largest=2).tolist() == \
        [True, True, False, False, False]
    none = MeshComponents(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert len(none) == 0 and none.select(min_fraction=0.5).shape == (0,)
    with pytest.raises(ValueError, match="one entry per vertex"):
        MeshComponents(labels, vc[:-1], fc)


def test_surface_mesh_filters_are_the_truths(truth_labels):
    from raynet_amd.volume import SurfaceMesh
    vertices, faces, normals, colors = _pieces(1)
    mesh = SurfaceMesh(vertices, faces, normals, colors)
    found = mesh.components()
    roots, component, n_vertices, n_faces = ct.dense(*ct.components(faces, len(vertices)))
    assert np.array_equal(found.roots, roots) and np.array_equal(found.n_faces, n_faces)
    assert len(roots) == 7 + 5 + 1 + 1 + 6 + 1 + 1
    for kw in (dict(keep_largest=1), dict(keep_largest=2), dict(keep_largest=4),
               dict(min_faces=4), dict(min_faces=5), dict(min_fraction=0.5),
               dict(min_fraction=0.25, keep_largest=3), dict(min_faces=10 ** 6)):
        got = mesh.without_small_components(**kw)
        want_v, want_f, used, _, _ = ct.filtered(vertices, faces, **kw)
        assert got is not mesh and got.faces.dtype == np.int32 and got.vertices.dtype == F
        assert np.array_equal(got.vertices.view(np.int32), want_v.view(np.int32)), kw
        assert np.array_equal(got.faces, want_f), kw
        assert np.array_equal(got.normals, normals[used]) and np.array_equal(got.colors, colors[used])
    # the mesh itself is what it was
    assert len(mesh.faces) == len(faces) and len(mesh.vertices) == len(vertices)
    # keep_components: ids, in any order and repeated, and masks
    for ids in ([0], [3, 1, 3], list(range(len(roots))), []):
        keep = np.zeros(len(roots), bool)
        keep[ids] = True
        want_v, want_f, used = ct.compact(vertices, faces, keep[component[faces[:, 0]]])
        for which in (ids, keep, np.array(ids, np.int64)):
            got = mesh.keep_components(which)
            assert np.array_equal(got.vertices.view(np.int32), want_v.view(np.int32))
            assert np.array_equal(got.faces, want_f) and np.array_equal(got.colors, colors[used])
    assert mesh.keep_components([]).empty
    with pytest.raises(ValueError, match="component id"):
        mesh.keep_components([len(roots)])
    with pytest.raises(ValueError, match="component id"):
        mesh.keep_components([-1])
    with pytest.raises(ValueError, match="mask over the components"):
        mesh.keep_components(np.ones(len(roots) + 1, bool))
    # the criteria
    with pytest.raises(ValueError, match="no criterion"):
        mesh.without_small_components()
    for kw, match in [(dict(min_faces=0), "min_faces"), (dict(keep_largest=0), "keep_largest"),
                      (dict(min_fraction=0.0), "min_fraction"), (dict(min_fraction=1.5), "min_fraction"),
                      (dict(min_fraction=float("nan")), "min_fraction")]:
        with pytest.raises(ValueError, match=match):
            mesh.without_small_components(**kw)
    # without attributes there are none afterwards
    bare = SurfaceMesh(vertices, faces).without_small_components(keep_largest=1)
    assert bare.normals is None and bare.colors is None and not bare.empty


def test_an_empty_mesh_stays_empty_without_the_gpu(truth_labels):
    from raynet_amd.volume import SurfaceMesh
    for mesh in (SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)),
                 SurfaceMesh(np.zeros((4, 3), F), np.zeros((0, 3), np.int32), np.zeros((4, 3), F))):
        out = mesh.without_small_components(keep_largest=1)
        assert out.empty and out.vertices.shape == (0, 3) and out.faces.shape == (0, 3)
        assert mesh.keep_components([]).empty
    assert truth_labels == []                      # nobody asked for labels
    with pytest.raises(ValueError, match="no criterion"):
        SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)).without_small_components()
    none = SurfaceMesh(np.zeros((0, 3), F), np.zeros((0, 3), np.int32)).components()
    assert len(none) == 0 and truth_labels == []


def test_the_flag_helper_filters_and_reports(truth_labels, capsys):
    from raynet_amd.scripts import fuse_depth_maps, mesh_flags
    from raynet_amd.volume import SurfaceMesh
    vertices, faces, _, _ = _pieces(2)
    mesh = SurfaceMesh(vertices, faces)
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply"])
    assert mesh_flags.drop_components(mesh, args) is mesh and capsys.readouterr().out == ""
    assert truth_labels == []
    args = fuse_depth_maps.build_parser().parse_args(["s", "p", "o.ply", "--min_component_faces", "4"])
    out = mesh_flags.drop_components(mesh, args)
    want_v, want_f, _, found, kept = ct.filtered(vertices, faces, min_faces=4)
    assert np.array_equal(out.faces, want_f)
    assert capsys.readouterr().out == "components: %d found, %d kept, %d -> %d faces\n" % (
        found, kept, len(faces), len(want_f))


# ------------------------------------------------------------------------------ the scripts
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
        assert a.min_component_faces is None and a.min_component_fraction is None
        assert a.keep_largest is None
        a = script.build_parser().parse_args(positional + [
            "--min_component_faces", "12", "--min_component_fraction", "0.25", "--keep_largest", "3"])
        assert (a.min_component_faces, a.min_component_fraction, a.keep_largest) == (12, 0.25, 3)
        for argv, message in [
                (["--min_component_faces", "0"], "--min_component_faces"),
                (["--min_component_faces", "-3"], "--min_component_faces"),
                (["--keep_largest", "0"], "--keep_largest"),
                (["--keep_largest", "-1"], "--keep_largest"),
                (["--min_component_fraction", "0"], "--min_component_fraction"),
                (["--min_component_fraction", "1.5"], "--min_component_fraction"),
                (["--min_component_fraction", "-0.5"], "--min_component_fraction"),
                (["--min_component_fraction", "nan"], "--min_component_fraction"),
                (["--min_component_fraction", "inf"], "--min_component_fraction")]:
            with pytest.raises(SystemExit) as e:
                script.main(positional + mesh_flag + argv)
            assert e.value.code == 2
            assert message in capsys.readouterr().err, (script.__name__, argv)
    # render_volume: the flags are the mesh's
    for argv, message in [(["--keep_largest", "1"], "--keep_largest"),
                          (["--min_component_faces", "5"], "--min_component_faces"),
                          (["--min_component_fraction", "0.5", "--mesh_cloud", out,
                            "--mesh_samples", "10"], "--min_component_fraction")]:
        with pytest.raises(SystemExit) as e:
            render_volume.main(cases[1][1] + argv)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert message in err and "--mesh" in err, argv
    assert not os.path.exists(out)
