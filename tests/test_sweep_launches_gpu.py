"""Every flavour of the plane sweep and of its planes -> voxels tail held PER LAUNCH to the float64
truth of tests/sweep_truth.py, at every entry of its output: k_sweep_map_packed with four and two
rays per wavefront, the cooperative k_sweep_map, the generic sweep (by option, by F, by N), odd
and even padding; MAPMODE 0 (rn_compute_similarities), SIM 0 + MAPMODE 1 (rn_planes_to_voxels),
sweep + MAPMODE 1 (rn_mvcnn_voxel_space) and MAPMODE 2 on packed lists (rn_scene_prepare) --
under features whose scores are flat, peaky, lifted past exp's overflow, and set apart between
neighbouring rays by more than exp's underflow: a softmax maximum taken over the wrong lanes, over
one chunk of planes, or not at all is the same column to rounding under flat features
(tests/test_sweep_truth.py holds that, and that the truth rejects each such mutant).  The bound is
derived in sweep_truth's docstring; no entry is excluded.  Out of scope: MAPMODE 3,
k_sweep_disparity, the range scheme (their own tests)."""
import numpy as np
import pytest

import sweep_truth as T

pytestmark = pytest.mark.gpu

CASES = T.launch_cases()
IDS = ["%s-%s" % (f, T.case_id(c)) + ("-rpw1" if o.get("sweep_rays_per_wave") else "") for f, o, c in CASES]
SENTINEL = -7.0
WORST = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    from raynet_amd import _lib
    _lib.build()
    yield torch
    for key in sorted(WORST):
        print("worst error / bound  %-12s %-8s %-20s %.3f" % (key + (WORST[key],)))


_TRUTH = {}


def _truth(oracle_mod, case):
    """The built case and its truths, computed once and shared by the entries (never modified)."""
    t = _TRUTH.get(case)
    if t is None:
        b = T.build(oracle_mod, case)
        col = T.column_truth(b.feats, b.idx, b.o.F)
        t = dict(b=b, S=col[0], tolS=col[1])
        _, _, t["Sv"], t["tolv"], _, _ = T.truths(b, column=col)
        _, _, t["Sv_fed"], t["tolv_fed"], _, _ = T.truths(b, chained=False, column=col)
        _, _, _, _, t["Sr"], t["tolr"] = T.truths(b, reciprocal=True, column=col)
        short = b.rvc <= 1
        assert short.sum() <= len(b.ridx) // 5              # the cap on rays the resident path skips
        _TRUTH[case] = t
    return t


def _ctx(torch, b, opts):
    from raynet_amd.hip_implementations import get_context
    from raynet_amd.hip_implementations.options import PathOptions
    o = b.o
    ctx = get_context(o.M, o.D, o.N, o.F, o.H, o.W, o.padding, o.bbox, o.grid_shape)
    ctx.set_voxel_grid(torch.from_numpy(b.vg).cuda())
    want = PathOptions(**opts)
    ctx.set_options(want)
    got = ctx.get_options()
    assert got["generic_sweep"] == want.generic_sweep
    assert got["sweep_rays_per_wave"] == want.sweep_rays_per_wave
    return ctx


def _reset(ctx):
    from raynet_amd.hip_implementations.options import PathOptions
    ctx.set_options(PathOptions())


def _record(flavour, case, entry, ratio):
    print("error / bound  %-12s %-30s %-20s %.3f" % (flavour, T.case_id(case), entry, ratio))
    key = (flavour, case.regime, entry)
    WORST[key] = max(WORST.get(key, 0.0), ratio)


def _mapped_ratio(got, b, Sv, tol, beyond):
    """Worst ratio over every entry of every ray with a voxel; the entries beyond `count` (the
    whole row of a ray without voxels) must hold `beyond`."""
    worst = 0.0
    for r in range(len(b.ridx)):
        cnt = int(b.rvc[r])
        assert np.all(got[r, cnt:] == beyond), r
        if cnt >= 1:
            worst = max(worst, T.worst_ratio(got[r, :cnt], Sv[r], tol[r]))
    return worst


@pytest.mark.parametrize("flavour,opts,case", CASES, ids=IDS)
def test_plane_column(torch, oracle_mod, flavour, opts, case):
    """rn_compute_similarities (MAPMODE 0)."""
    t = _truth(oracle_mod, case)
    b = t["b"]
    ctx = _ctx(torch, b, opts)
    S = torch.full((len(b.ridx), b.o.D), SENTINEL, device="cuda")
    try:
        ctx.compute_similarities(ctx.dev(b.feats), ctx.dev(b.P), ctx.dev(b.starts), ctx.dev(b.ends), S)
    finally:
        _reset(ctx)
    S = S.cpu().numpy()
    ratio = T.worst_ratio(S, t["S"], t["tolS"])
    _record(flavour, case, "compute_similarities", ratio)
    assert np.isfinite(S).all()
    assert ratio <= 1.0


@pytest.mark.parametrize("flavour,opts,case", CASES, ids=IDS)
def test_planes_to_voxels_fed_with_the_truth(torch, oracle_mod, flavour, opts, case):
    """rn_planes_to_voxels (SIM 0, MAPMODE 1) on the float64 column rounded to fp32."""
    t = _truth(oracle_mod, case)
    b = t["b"]
    n = len(b.ridx)
    ctx = _ctx(torch, b, opts)
    Sv = torch.zeros((n, b.o.M), device="cuda")
    try:
        ctx.planes_to_voxels(ctx.dev(b.rvi), ctx.dev(b.rvc), ctx.dev(b.starts), ctx.dev(b.ends),
                             ctx.dev(t["S"].astype(np.float32)), Sv)
    finally:
        _reset(ctx)
    ratio = _mapped_ratio(Sv.cpu().numpy(), b, t["Sv_fed"], t["tolv_fed"], 0.0)
    _record(flavour, case, "planes_to_voxels", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("flavour,opts,case", CASES, ids=IDS)
def test_voxel_space_from_cameras(torch, oracle_mod, flavour, opts, case):
    """rn_mvcnn_voxel_space (traversal, sweep, MAPMODE 1): the oracle's lists, the chained truth."""
    t = _truth(oracle_mod, case)
    b = t["b"]
    n = len(b.ridx)
    ctx = _ctx(torch, b, opts)
    rvi = torch.zeros((n, b.o.M, 3), dtype=torch.int32, device="cuda")
    rvc = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    Sv = torch.zeros((n, b.o.M), device="cuda")
    try:
        ctx.mvcnn_voxel_space(ctx.dev(b.ridx), ctx.dev(b.feats), ctx.dev(b.P), ctx.dev(b.P_inv),
                              ctx.dev(b.center), rvi, rvc, Sv)
    finally:
        _reset(ctx)
    assert np.array_equal(rvc.cpu().numpy(), b.rvc) and np.array_equal(rvi.cpu().numpy(), b.rvi)
    ratio = _mapped_ratio(Sv.cpu().numpy(), b, t["Sv"], t["tolv"], 0.0)
    _record(flavour, case, "mvcnn_voxel_space", ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("rays_per_wave", [0, 1])
@pytest.mark.parametrize("flavour,opts,case", CASES, ids=IDS)
def test_resident_prepare(torch, oracle_mod, flavour, opts, case, rays_per_wave):
    """rn_scene_prepare (MAPMODE 2, packed lists staged by LDS-DMA, hardware reciprocal and
    v_exp_f32), under both sweep_rays_per_wave settings.  A ray with <= 1 voxels is never read on
    the resident path (raynet_hip.h): its row of Sr is not written, its list and count are."""
    if opts.get("sweep_rays_per_wave") == 1 and rays_per_wave == 0:
        opts = {k: v for k, v in opts.items() if k != "sweep_rays_per_wave"}
    elif rays_per_wave == 1:
        opts = dict(opts, sweep_rays_per_wave=1)
    t = _truth(oracle_mod, case)
    b = t["b"]
    n, M = len(b.ridx), b.o.M
    ctx = _ctx(torch, b, opts)
    f_d = ctx.dev(b.feats)
    vox = torch.zeros((n, M), dtype=torch.int32, device="cuda")
    rvc = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    Sr = torch.full((n, M), SENTINEL, device="cuda")
    try:
        ctx.scene_prepare(ctx.dev(b.ridx), [f_d[v] for v in range(b.o.N)], ctx.dev(b.P),
                          ctx.dev(b.P_inv), ctx.dev(b.center), vox, rvc, Sr)
    finally:
        _reset(ctx)
    vox, rvc, Sr = T.unpack_voxels(vox.cpu().numpy()), rvc.cpu().numpy(), Sr.cpu().numpy()
    assert np.array_equal(rvc, b.rvc)
    worst = 0.0
    for r in range(n):
        cnt = int(b.rvc[r])
        assert np.array_equal(vox[r, :cnt], b.rvi[r, :cnt]), r
        if cnt <= 1:
            assert np.all(Sr[r] == SENTINEL), r             # never written, never read
            continue
        assert np.all(Sr[r, cnt:] == SENTINEL), r
        worst = max(worst, T.worst_ratio(Sr[r, :cnt], t["Sr"][r], t["tolr"][r]))
    _record(flavour, case, "scene_prepare rpw=%d" % rays_per_wave, worst)
    assert worst <= 1.0
