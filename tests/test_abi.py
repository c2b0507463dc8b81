"""CPU-side checks of the drop-in boundary: libraynet_hip.so builds for gfx950, loads,
and exports every symbol include/raynet_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

import abi_header
from conftest import REPO


def _declared_symbols():
    text = open(os.path.join(REPO, "include", "raynet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rn_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_header_symbols():
    from raynet_amd import _lib
    path = _lib.build()
    lib = ctypes.CDLL(path)
    names = _declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "missing export %s" % n
    assert sorted(_lib.SIGNATURES) == names     # the ctypes table covers the whole header
    _lib.load()
    # the shipped library is the DEFAULT build: no exact-arithmetic / statistics / A-B knob and no
    # extra compiler flag went into it (rn_version() names every one that did)
    lib.rn_version.restype = ctypes.c_char_p
    version = lib.rn_version().decode()
    assert version.startswith("raynet_hip") and version.endswith("knobs: | extra:"), version


@pytest.mark.parametrize("name", sorted(abi_header.prototypes()))
def test_every_entry_is_bound_as_the_header_declares_it(name):
    """Arity, every argument type and the return type: in the table, and on the function object
    of the loaded library."""
    from raynet_amd import _lib
    returns, declared = abi_header.prototype(name)
    assert name in _lib.SIGNATURES, "%s has no entry in _lib.SIGNATURES" % name
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(declared), (name, len(sig), declared)
    for k, (arg, ctype) in enumerate(zip(declared, sig)):
        assert ctype is abi_header.argtype_of(arg, ctype), (name, k, arg, ctype)
    restype = abi_header.restype_of(returns)
    assert _lib.RETURNS.get(name, ctypes.c_int) is restype, (name, returns)
    assert (name in _lib.RETURNS) == (returns != "int"), (name, returns)
    _lib.build()
    fn = getattr(_lib.load(), name)
    assert list(fn.argtypes) == sig and fn.restype is restype, (name, fn.argtypes, fn.restype)


def test_the_header_parser_refuses_what_it_does_not_know():
    for arg in ("size_t n", "rn_config cfg", "rn_ctx ctx", "void stream", "int32_t", "float (*f)(int)",
                "rn_options **out"):
        with pytest.raises(ValueError):
            abi_header.argtype_of(arg)
    with pytest.raises(ValueError):
        abi_header.restype_of("float")
    assert abi_header.argtype_of("const double cell[3]") is ctypes.c_void_p
    assert abi_header.argtype_of("uint32_t *views", ctypes.POINTER(ctypes.c_uint32)) is \
        ctypes.POINTER(ctypes.c_uint32)
    assert abi_header.argtype_of("uint32_t *views", ctypes.POINTER(ctypes.c_int32)) is ctypes.c_void_p
    assert abi_header.argtype_of("int64_t *counts", ctypes.POINTER(ctypes.c_int64)) is ctypes.c_void_p


def test_the_sources_are_the_files_of_csrc_and_the_header():
    from raynet_amd import _lib
    srcs = _lib.sources()
    assert srcs[0] == os.path.join(_lib.CSRC, "raynet_hip.hip") and srcs[-1] == _lib.HEADER
    found = sorted(os.path.join(_lib.CSRC, f) for f in os.listdir(_lib.CSRC)
                   if f.endswith((".hip", ".inl", ".h")))
    assert sorted(srcs[:-1]) == found and len(set(srcs)) == len(srcs) >= 39
    assert srcs[1:-1] == sorted(srcs[1:-1])
    assert not any(s.endswith(".so") for s in srcs)


def test_build_is_stale_when_any_one_source_is_newer(monkeypatch, tmp_path):
    """No compile: the compiler call is caught, and the times are a table."""
    from raynet_amd import _lib
    monkeypatch.delenv("RAYNET_HIPCC_EXTRA", raising=False)
    target = str(tmp_path / "libvariant.so")
    open(target, "w").close()
    calls = []
    monkeypatch.setattr(_lib.subprocess, "check_call", lambda cmd, cwd=None: calls.append(cmd))
    for newer in [None] + _lib.sources():
        monkeypatch.setattr(_lib.os.path, "getmtime", lambda p: 2.0 if p == newer else 1.0)
        del calls[:]
        assert _lib.build(out=target) == target
        assert len(calls) == (0 if newer is None else 1), newer
    # the compile line: the translation unit alone, the flags, the target
    assert calls[0] == [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + _lib.HIPCC_FLAGS + \
        [_lib.sources()[0], "-o", target]


def test_no_timing_only_branches_in_the_product_sources():
    """The ablation switches of earlier rounds (results wrong on purpose) live in
    tools/experiments/ as a patch; the translation unit that ships has none."""
    csrc = os.path.join(REPO, "raynet_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h", ".inl")):
            src = open(os.path.join(csrc, f)).read()
            assert "RN_EXP" not in src and "wrong results" not in src.lower(), f


def test_the_only_build_switches_are_the_exact_arithmetic_ones():
    """Round 6: every A/B switch of the laboratory (phase-stop instrumentation, literal forms kept
    next to their exact shortcuts, tile / block / chunk knobs) left the product sources as
    tools/experiments/r06_lab_switches_removed.patch; what may still be conditional is the
    exact-arithmetic build tests/test_exact_build_gpu.py keeps under test and the build tag."""
    import re
    csrc = os.path.join(REPO, "raynet_amd", "csrc")
    allowed = {"RN_EXACT_OCC_EXP", "RN_EXACT_SOFTMAX_EXP", "RN_EXACT_BP_MATH", "RN_BUILD_EXTRA"}
    count = 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h", ".inl")):
            continue
        for line in open(os.path.join(csrc, f)):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                count += 1
                names = set(re.findall(r"\bRN_[A-Z0-9_]+", line))
                assert names and names <= allowed, (f, line)
    assert count <= 15, count


def test_no_device_is_an_error_not_a_fallback():
    """Without a GPU the product refuses to run (there is no CPU route)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import HipContext
    with pytest.raises(_lib.RaynetHipError):
        HipContext(32, 8, 2, 4, 8, 8, 3, (0, 0, 0, 1, 1, 1), (4, 4, 4))
    lib = _lib.load()
    cfg = _lib.Config()
    cfg.M, cfg.D, cfg.N, cfg.F, cfg.H, cfg.W, cfg.padding = 32, 8, 2, 4, 8, 8, 3
    for i in range(3):
        cfg.grid[i] = 4
        cfg.bbox[3 + i] = 1.0
    h = ctypes.c_void_p()
    assert lib.rn_create(ctypes.byref(cfg), ctypes.byref(h)) == -3     # RN_ERR_NO_DEVICE


def test_product_package_never_touches_the_oracle():
    """raynet_amd must not import / link / open anything under oracle/ (comments may
    mention it)."""
    bad = re.compile(r"(^|\s)(import|from)\s+oracle\b|libraynet_oracle|oracle/|oracle\.\w+\(|rno_\w+\(",
                     re.M)
    pkg = os.path.join(REPO, "raynet_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(root, f)).read()
                m = bad.search(src)
                assert m is None, "%s references the oracle: %r" % (f, m.group(0))


def test_host_side_mirrors_reference_names():
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import (ForwardPass, MultiViewCNNForwardPass,
                                         MultiViewCNNVoxelSpaceForwardPass, RayNetForwardPass,
                                         get_forward_pass_factory, shard_bounds)
    assert get_forward_pass_factory("raynet") is RayNetForwardPass
    assert get_forward_pass_factory("multi_view_cnn") is MultiViewCNNForwardPass
    assert get_forward_pass_factory("multi_view_cnn_voxel_space") is MultiViewCNNVoxelSpaceForwardPass
    assert issubclass(RayNetForwardPass, ForwardPass)
    gp = GenerationParameters()
    assert gp.depth_planes == 32 and gp.neighbors == 4 and gp.max_number_of_marched_voxels == 400
    # every ray owned by exactly one rank, in order
    for n in (0, 1, 7, 307200):
        for world in (1, 2, 3, 8):
            b = [shard_bounds(n, r, world) for r in range(world)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(b[i][1] == b[i + 1][0] for i in range(world - 1))


def test_scene_shim_conventions():
    import numpy as np
    from raynet_amd.common.scene import adjacent_views, get_voxel_grid
    from oracle.oracle import voxel_grid_centers
    g = get_voxel_grid(np.array([[-1, -1, -1, 1, 1, 1]], np.float32), (8, 4, 2))
    assert g.shape == (3, 8, 4, 2) and g.dtype == np.float32
    assert np.array_equal(np.ascontiguousarray(g.transpose(1, 2, 3, 0)),
                          voxel_grid_centers([-1, -1, -1, 1, 1, 1], (8, 4, 2)))
    assert np.allclose(g[0, :, 0, 0], -1 + (np.arange(8) + 0.5) * 0.25)
    assert adjacent_views(0, 12, 4) == [1, 2, 3, 4]
    assert adjacent_views(11, 12, 4) == [7, 8, 9, 10]
    assert adjacent_views(5, 12, 4) == [3, 4, 6, 7]
    assert adjacent_views(2, 5, 4) == [0, 1, 3, 4]
