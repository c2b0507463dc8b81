"""Parity of the HIP path (through the C ABI) with the CPU oracle and with the
golden vectors generated from the reference.  Needs a real MI355X: `-m gpu`.

Bar (north_star / SURVEY.md Q8): ray<->voxel index maps, ray end points and plane
indices bit-exact; distributions <= 1e-5 abs; log-odds messages / accumulators
within the fp32 conditioning bound; depth maps within 1e-4 except documented
arg-max near-ties."""
import numpy as np
import pytest

from bp_truth import bp_truth_f64 as _bp_truth_f64
from conftest import assert_depth_flips_are_near_ties, load_cases

pytestmark = pytest.mark.gpu

# crosscheck_cu_host.npz: seeded CASES (cameras, rays, shapes) with outputs of an earlier host-side
# run of the reference's .cu text behind `#define` stand-ins.  It PINS NOTHING: the
# comparator of every test below is the oracle (pinned stage by stage); where a
# stored output is also compared it is a second, weaker look.  The reference's own kernels, compiled
# unchanged for gfx950, are the a2 pin: tests/test_reference_kernels.py.
CU = load_cases("crosscheck_cu_host.npz")
TRAV = load_cases("ref_traversal.npz")
MRF = load_cases("ref_mrf_np.npz")
MAP = load_cases("ref_mapping_np.npz")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    from raynet_amd import _lib
    _lib.build()
    return torch


def logit_tol(ref_msg):
    return 1e-5 + 8 * 2.0 ** -24 * np.exp(np.minimum(np.abs(ref_msg), 17.0))


def make_case(oracle_mod, c):
    o = oracle_mod.Oracle(M=int(c["M"]), D=int(c["D"]), N=int(c["N"]), F=int(c["F"]),
                          H=int(c["H"]), W=int(c["W"]), padding=int(c["padding"]),
                          bbox=c["bbox"], grid_shape=c["grid"])
    rng = np.random.default_rng(int(c["seed"]))
    feats = rng.standard_normal((o.N, o.H + o.padding + 1, o.W + o.padding + 1, o.F),
                                dtype=np.float32) * np.float32(0.25)
    vg = oracle_mod.voxel_grid_centers(c["bbox"], c["grid"])
    return o, feats, vg


def hip_ctx(o):
    from raynet_amd.hip_implementations import get_context
    return get_context(o.M, o.D, o.N, o.F, o.H, o.W, o.padding, o.bbox, o.grid_shape)


# ------------------------------------------------------------------ a1
@pytest.mark.parametrize("case", sorted(CU))
def test_sample_rays_bit_exact(torch, oracle_mod, case):
    c = CU[case]
    o, _, _ = make_case(oracle_mod, c)
    ctx = hip_ctx(o)
    ridx = ctx.dev(c["ray_idxs"])
    n = len(ridx)
    s = torch.zeros((n, 3), device="cuda")
    e = torch.zeros((n, 3), device="cuda")
    ctx.sample_rays(ridx, ctx.dev(c["P_inv"]), ctx.dev(c["center"]), s, e)
    so, eo = o.sample(c["ray_idxs"], c["P_inv"], c["center"])
    assert np.array_equal(s.cpu().numpy(), so) and np.array_equal(e.cpu().numpy(), eo)
    assert np.array_equal(so, c["starts"]) and np.array_equal(eo, c["ends"])


def test_sample_points_k8(torch, oracle_mod):
    """K8 (sample_points.py:12-54): D points per ray, homogeneous coordinate 1."""
    from raynet_amd.hip_implementations.sample_points import batch_sample_points
    c = CU["small"]
    o, _, _ = make_case(oracle_mod, c)
    sp = batch_sample_points(o.D, o.H, o.W, o.bbox, "sample_in_bbox")
    pts = torch.zeros((len(c["ray_idxs"]), o.D, 4), device="cuda")
    sp(c["ray_idxs"], c["P_inv"], c["center"], pts)
    pts = pts.cpu().numpy()
    s, e = c["starts"], c["ends"]
    k = np.arange(o.D, dtype=np.float32)[None, :, None]
    expect = s[:, None, :] + k * (e - s)[:, None, :] / np.float32(o.D - 1)
    assert np.array_equal(pts[..., :3], expect.astype(np.float32))
    assert np.all(pts[..., 3] == 1.0)


# ------------------------------------------------------------------ a2
@pytest.mark.parametrize("case", sorted(CU))
@pytest.mark.parametrize("generic", [False, True])
def test_similarities(torch, oracle_mod, case, generic):
    """K7.  The generic sweep walks the dot product in the reference's order (equal to
    the oracle up to expf); the cooperative F=32 sweep re-associates the 32-term sums.
    (Flat features, an absolute bar: the accuracy of the values, per flavour and under features
    that show a wrong softmax maximum, is tests/test_sweep_launches_gpu.py.)"""
    from raynet_amd.hip_implementations.options import PathOptions
    c = CU[case]
    o, feats, _ = make_case(oracle_mod, c)
    ctx = hip_ctx(o)
    # (contexts are cached per shape: the option is SET on it, an environment variable read at
    # rn_create would only reach the first test that creates the context)
    ctx.set_options(PathOptions(generic_sweep=generic))
    assert ctx.get_options()["generic_sweep"] == generic
    n = len(c["ray_idxs"])
    S = torch.zeros((n, o.D), device="cuda")
    try:
        ctx.compute_similarities(ctx.dev(feats), ctx.dev(c["P"]), ctx.dev(c["starts"]),
                                 ctx.dev(c["ends"]), S)
    finally:
        ctx.set_options(PathOptions())
    So = o.similarities(feats, c["P"], c["starts"], c["ends"])
    S = S.cpu().numpy()
    assert np.abs(S.sum(1) - 1).max() < 1e-5
    tol = 2e-6 if (generic or o.F != 32) else 1e-5
    assert np.abs(S - So).max() <= tol
    assert np.abs(S - c["S"]).max() <= tol        # (the stored host-side run: no pin, see the top)


def test_similarities_beyond_64_kb_of_lds_in_two_contexts(torch, oracle_mod):
    """A sweep whose workgroup needs more than 64 KB of dynamic LDS has to opt in per kernel
    (hipFuncSetAttribute), and a context keeps for itself which kernels it has opted in: 32^3
    voxels, M = 256, D = 3072 take 4 * (96 + 3076 + 4 * (3072 + 256)) = 65,936 bytes.  Two contexts
    of that shape, created one after the other, both run K7, agree bit for bit and meet the oracle.
    Both are on device 0: this holds the per-context path, it does not reproduce what a second
    DEVICE did to the process-wide record this replaced."""
    from raynet_amd.hip_implementations.context import HipContext
    c = CU["wide"]
    grid, M, D = (32, 32, 32), 256, 3072
    assert 4 * (sum(grid) + (D + 4) // 4 * 4 + 4 * (D + M)) == 65936 > 64 * 1024
    o = oracle_mod.Oracle(M=M, D=D, N=int(c["N"]), F=int(c["F"]), H=int(c["H"]), W=int(c["W"]),
                          padding=int(c["padding"]), bbox=c["bbox"], grid_shape=grid)
    assert o.F == 32                              # the cooperative sweep
    rng = np.random.default_rng(int(c["seed"]))
    feats = rng.standard_normal((o.N, o.H + o.padding + 1, o.W + o.padding + 1, o.F),
                                dtype=np.float32) * np.float32(0.25)
    So = o.similarities(feats, c["P"], c["starts"], c["ends"])
    out = []
    for k in range(2):
        ctx = HipContext(M, D, o.N, o.F, o.H, o.W, o.padding, o.bbox, grid)
        S = torch.zeros((len(c["starts"]), D), device="cuda")
        ctx.compute_similarities(ctx.dev(feats), ctx.dev(c["P"]), ctx.dev(c["starts"]),
                                 ctx.dev(c["ends"]), S)
        out.append((ctx, S.cpu().numpy()))        # (the first context lives on while the second runs)
    assert np.array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][1] - So).max() <= 1e-5   # test_similarities' bar for the cooperative sweep


# ------------------------------------------------------------------ a3
@pytest.mark.parametrize("case", sorted(TRAV))
def test_traversal_bit_exact_vs_reference_cython(torch, oracle_mod, case):
    """K5 against index maps produced by the reference's compiled Cython traversal."""
    from raynet_amd.ray_marching.ray_tracing_hip import batch_voxel_traversal
    c = TRAV[case]
    M = int(c["M"])
    vtr = batch_voxel_traversal(M, c["bbox"], c["grid"])
    n = len(c["starts"])
    rvi = torch.zeros((n, M, 3), dtype=torch.int32, device="cuda")
    rvc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    vtr(c["starts"], c["ends"], rvi, rvc)
    assert np.array_equal(rvc.cpu().numpy(), c["rvc"])          # 0 is written explicitly (Q11)
    assert np.array_equal(rvi.cpu().numpy(), c["rvi"].astype(np.int32))


def test_traversal_reference_unit_tests(torch):
    """tests/test_ray_marching.py:20-102 run against the drop-in single-ray signature."""
    from raynet_amd.ray_marching.ray_tracing_hip import voxel_traversal
    bbox = np.array([3, 3, 0, 6, 6, 1], dtype=np.float32)
    grid_shape = np.array([3, 3, 1], dtype=np.int32)
    voxels = np.empty((10, 3), dtype=np.int32)
    voxels.fill(0)
    N = voxel_traversal(bbox, grid_shape, voxels, np.array([3., 4.1, 0.5], dtype=np.float32),
                        np.array([6., 4.9, 0.5], dtype=np.float32))
    assert N == 3
    assert np.all(voxels[:3, 1] == 1) and np.all(voxels[:3, 0] == np.arange(3))
    for s, e, cnt in [([4., 6., .5], [6., 5., .5], 2), ([3., 3., .5], [6., 6., .5], 5),
                      ([6., 6., .5], [3., 3., .5], 5)]:
        voxels.fill(0)
        assert voxel_traversal(bbox, grid_shape, voxels, np.array(s, np.float32),
                               np.array(e, np.float32)) == cnt
    bbox = np.array([0, 0, 0, 6, 6, 1], dtype=np.float32)
    grid_shape = np.array([6, 6, 1], dtype=np.int32)
    rvi = np.zeros((10, 3), dtype=np.int32)
    Nr = voxel_traversal(bbox, grid_shape, rvi, np.array([0., 3.5, 0.5], dtype=np.float32),
                         np.array([6., 0.5, 0.5], dtype=np.float32))
    assert Nr == 9
    assert np.all(rvi == np.array([[0, 3, 0], [0, 2, 0], [1, 2, 0], [2, 2, 0], [2, 1, 0], [3, 1, 0],
                                   [4, 1, 0], [4, 0, 0], [5, 0, 0], [0, 0, 0]]))
    bbox = np.array([-3., -3., -0.5, 3., 3., 2.], dtype=np.float32)
    grid_shape = np.array([32, 32, 10], dtype=np.int32)
    voxels = np.zeros((100, 3), dtype=np.int32)
    N = voxel_traversal(bbox, grid_shape, voxels,
                        np.array([-1.40056884, -1.34645462, 2.], dtype=np.float32),
                        np.array([-2.30040455, 3., -0.37297964], dtype=np.float32))
    assert N < 50


def test_traversal_large_random_vs_oracle(torch, oracle_mod):
    """20k chords through 128^3 (M=384), including truncation at M, vs the oracle."""
    from raynet_amd.ray_marching.ray_tracing_hip import batch_voxel_traversal
    rng = np.random.default_rng(3)
    bbox = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    grid = np.array([128, 128, 128], np.int32)
    n = 20000
    starts = (rng.random((n, 3)) * 2.4 - 1.2).astype(np.float32)
    ends = (rng.random((n, 3)) * 2.4 - 1.2).astype(np.float32)
    for M in (384, 64):
        o = oracle_mod.Oracle(M=M, D=8, N=2, F=4, H=4, W=4, padding=3, bbox=bbox, grid_shape=grid)
        vtr = batch_voxel_traversal(M, bbox, grid)
        rvi = torch.zeros((n, M, 3), dtype=torch.int32, device="cuda")
        rvc = torch.zeros((n,), dtype=torch.int32, device="cuda")
        vtr(starts, ends, rvi, rvc)
        rvi_o, rvc_o = o.traversal(starts, ends)
        assert np.array_equal(rvc.cpu().numpy(), rvc_o)
        assert np.array_equal(rvi.cpu().numpy(), rvi_o)
        if M == 64:
            assert (rvc_o == M).any()       # silent truncation at M (ray_tracing.cu:100)


# ------------------------------------------------------------------ a4
@pytest.mark.parametrize("case", sorted(CU))
def test_mapping_vs_oracle(torch, oracle_mod, case):
    """K6 on real traversals: plane walk reproduced exactly, values to fp32 rounding."""
    from raynet_amd.planes_voxels_mapping.planes_voxels_mapping_hip import \
        batch_depth_to_voxels_mapping
    c = CU[case]
    o, feats, vg = make_case(oracle_mod, c)
    pvm = batch_depth_to_voxels_mapping(o.M, o.D, o.grid_shape, o.bbox)
    rvi = c["rvi"].astype(np.int32)
    n = len(rvi)
    out = torch.zeros((n, o.M), device="cuda")
    pvm(vg, rvi, c["rvc"], c["starts"], c["ends"], c["S"], out)
    out = out.cpu().numpy()
    ref = o.planes_to_voxels(vg, rvi, c["rvc"], c["starts"], c["ends"], c["S"])
    assert np.abs(out - ref).max() <= 2e-7
    assert np.abs(out - c["S_voxel"]).max() <= 2e-7
    for r in range(n):
        assert np.all(out[r, c["rvc"][r]:] == 0)


@pytest.mark.parametrize("case", sorted(MAP))
def test_mapping_vs_reference_numpy(torch, case):
    """K6 vs the reference's NumPy `li` / `li_2` (planes_voxels_mapping.py:122-211)."""
    from raynet_amd.planes_voxels_mapping.planes_voxels_mapping_hip import \
        batch_depth_to_voxels_mapping
    c = MAP[case]
    C, D = len(c["voxels"]), len(c["s"])
    if D < 2:
        pytest.skip("D=1 undefined")
    M = C + 3
    pvm = batch_depth_to_voxels_mapping(M, D, (C, 1, 1))
    grid = np.zeros((C, 1, 1, 3), np.float32)
    grid[:, 0, 0, :] = c["voxels"]
    rvi = np.zeros((1, M, 3), np.int32)
    rvi[0, :C, 0] = np.arange(C)
    out = torch.zeros((1, M), device="cuda")
    pvm(grid, rvi, np.array([C], np.int32), c["start"][None], c["end"][None], c["s"][None], out)
    out = out.cpu().numpy()
    assert np.allclose(out[0, :C], c["li"], rtol=2e-5, atol=1e-7)
    assert np.allclose(out[0, :C], c["li_2"], rtol=2e-5, atol=1e-7)
    assert np.all(out[0, C:] == 0)


# ---------------------------------------------------------------- a5 / a6 / a9
class _GP(object):
    def __init__(self, grid_shape, M):
        self.grid_shape = grid_shape
        self.max_number_of_marched_voxels = M


@pytest.mark.parametrize("case", sorted(MRF))
def test_bp_backend_vs_reference_numpy(torch, oracle_mod, case):
    """get_bp_backend("hip") through the reference's BPInference interface, against
    outputs of mrf/mrf_np.py (accumulator, messages, depth distribution) and the oracle."""
    from raynet_amd.mrf.bp_inference import get_bp_backend
    c = MRF[case]
    N, M = c["S"].shape
    bp = get_bp_backend("hip", _GP(c["grid"], M), bp_iterations=3, batch_size=max(1, N // 2))
    init = np.random.default_rng(0).random((N, M)).astype(np.float32)   # ignored, like the reference
    acc, msgs = bp.update_bp_messages(c["S"], c["rvi"], c["rvc"], init)
    prior = np.float32(np.log(0.05) - np.log(0.95))
    assert np.all(np.abs(acc - c["accs"][-1]) <= logit_tol(c["accs"][-1] - prior) * 4)
    assert np.all(np.abs(msgs - c["msgs"]) <= logit_tol(c["msgs"]))
    S_new = bp.estimate_depth_probabilities_from_messages(
        c["S"], c["rvi"], c["rvc"], acc, msgs, np.zeros_like(c["S"]))
    assert np.abs(S_new - c["S_new"]).max() < 1e-5
    skip = c["rvc"] <= 1
    assert np.all(msgs[skip] == 0) and np.all(S_new[skip] == 0)
    # and the fp32 oracle (same arithmetic up to scan association / expf / logf)
    o = oracle_mod.Oracle(M=M, D=8, N=2, F=4, H=4, W=4, padding=3, bbox=(0, 0, 0, 1, 1, 1),
                          grid_shape=c["grid"])
    acc_o, msgs_o = o.belief_propagation(c["S"], c["rvi"], c["rvc"], np.zeros_like(c["S"]))
    assert np.all(np.abs(msgs - msgs_o) <= logit_tol(msgs_o))


def test_bp_single_sweep_against_float64_truth(torch, oracle_mod):
    """Saturated regime (|accumulator| up to 40 log-odds, peaked columns): the HIP sweep
    stays within fp32 rounding x logit conditioning of the float64 value, and never
    produces a non-finite message.  The oracle (reference arithmetic) is held to the
    same bound plus the cancellation term of its (cumsum1 - cumsum2), mrf_bp.cu:157."""
    from raynet_amd.mrf.mrf_hip import batch_ray_belief_propagation
    rng = np.random.default_rng(42)
    grid, M, n = (32, 32, 32), 96, 400
    bbox = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    o = oracle_mod.Oracle(M=M, D=8, N=2, F=4, H=4, W=4, padding=3, bbox=bbox, grid_shape=grid)
    starts = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    ends = (rng.random((n, 3)) * 2 - 1).astype(np.float32)
    axis = rng.integers(0, 3, n)
    starts[np.arange(n), axis] = -1
    ends[np.arange(n), axis] = 1
    rvi, rvc = o.traversal(starts, ends)
    S = np.zeros((n, M), np.float32)
    for r in range(n):
        c = rvc[r]
        v = rng.random(c) ** 6 + 1e-6
        v[rng.integers(0, c)] += rng.random() * 5
        S[r, :c] = v / v.sum()
    acc = (rng.random(grid) * 80 - 40).astype(np.float32)
    msgs_in = (rng.random((n, M)) * 6 - 3).astype(np.float32)
    truth, cancel = _bp_truth_f64(S, rvi, rvc, acc, msgs_in)
    valid = np.arange(M)[None, :] < rvc[:, None]
    eps = 2.0 ** -24
    cond = 2 + np.exp(np.minimum(np.abs(truth), 30))
    bp, _ = batch_ray_belief_propagation(M, grid)
    m_hip = torch.from_numpy(msgs_in.copy()).cuda()
    acc_out = torch.zeros(grid, device="cuda")
    bp(S, rvi, rvc, acc, m_hip, acc_out)
    m_hip = m_hip.cpu().numpy()
    assert np.isfinite(m_hip).all()
    # (1 - o) carries a relative error eps/(1-o) <= 6e-4 once o saturates at its clamp
    tol_hip = 1e-3 + 32 * eps * cond
    ratio = np.where(valid, np.abs(m_hip - truth) / tol_hip, 0)
    wr, wi = np.unravel_index(ratio.argmax(), ratio.shape)
    m_dbg = msgs_in.copy()
    o.bp_sweep(S, rvi, rvc, acc, m_dbg, np.zeros(grid, np.float32))
    assert ratio.max() <= 1, "ray %d (count %d) idx %d: hip %g truth %g oracle %g ratio %g; n_bad %d" % (
        wr, rvc[wr], wi, m_hip[wr, wi], truth[wr, wi], m_dbg[wr, wi], ratio.max(), (ratio > 1).sum())
    # scatter-add of exactly these messages
    ref_acc = np.zeros(grid, np.float64)
    for r in range(n):
        np.add.at(ref_acc, tuple(rvi[r, :rvc[r]].T), m_hip[r, :rvc[r]].astype(np.float64))
    assert np.abs(acc_out.cpu().numpy() - ref_acc).max() <= 1e-3
    # the reference arithmetic on the same inputs
    m_o = msgs_in.copy()
    o.bp_sweep(S, rvi, rvc, acc, m_o, np.zeros(grid, np.float32))
    fin = np.isfinite(m_o) & valid
    tol_o = 1e-3 + 32 * eps * cond + 8 * eps * cancel
    assert np.all(np.abs(m_o - truth)[fin] <= tol_o[fin])
    # where the reference is well conditioned the two fp32 paths agree closely
    easy = fin & (cancel < 1e3) & (np.abs(truth) < 8)
    assert easy.sum() > 0.3 * valid.sum()
    assert np.abs(m_hip - m_o)[easy].max() <= 2e-3


def _occupancy(acc):
    mx = np.maximum(0.0, acc)
    t1, t2 = np.exp(0.0 - mx), np.exp(acc - mx)
    return t2 / (t2 + t1)


def test_bp_reference_property_tests(torch):
    """tests/test_mrf.py (:73-76, :140-144, :213-215, :281-304, :349, :414-416) with the
    HIP backend in place of numpy/tf/cuda."""
    from raynet_amd.mrf.bp_inference import get_bp_backend
    res = {}
    for case in ("single_ray", "two_rays", "two_rays_2", "three_rays", "conflict"):
        c = MRF[case]
        N, M = c["S"].shape
        bp = get_bp_backend("hip", _GP(c["grid"], M), bp_iterations=3, batch_size=N)
        acc, msgs = bp.update_bp_messages(c["S"], c["rvi"], c["rvc"],
                                          np.random.random((N, M)).astype(np.float32))
        res[case] = (bp, c, acc, msgs, _occupancy(acc))
    p = res["single_ray"][4]
    ix = np.where(p == p.max())
    assert ix[0][0] == 2 and ix[1][0] == 2
    p = res["two_rays"][4].T
    assert max(p[0, 4, 3], p[0, 2, 2]) >= p.max() - 1e-12
    p = res["two_rays_2"][4].T
    assert p[0, 2, 2] >= p.max() - 1e-12
    p = res["three_rays"][4].T
    order = np.sort(p[0].ravel())[::-1]
    assert p[0, 2, 2] == order[0] and p[0, 2, 0] == order[1] and p[0, 4, 4] == order[2]
    bp, c, acc, msgs, p = res["conflict"]
    assert p.T[0, 0, 2] < 0.1
    S_new = bp.estimate_depth_probabilities_from_messages(c["S"], c["rvi"], c["rvc"], acc, msgs,
                                                          np.zeros_like(c["S"]))
    assert S_new[0, 2] < 0.5 and S_new[0, 6] > 0.9 and S_new[1, 4] > 0.9


def test_mrf_inference_and_errors(torch):
    from raynet_amd.mrf.bp_inference import get_bp_backend
    c = MRF["rand32"]
    N, M = c["S"].shape
    bp = get_bp_backend("hip", _GP(c["grid"], M), batch_size=N)
    acc, msgs, S_new = bp.mrf_inference(c["S"], c["rvi"], c["rvc"], np.zeros_like(c["S"]),
                                        np.zeros_like(c["S"]))
    assert np.abs(S_new - c["S_new"]).max() < 1e-5
    with pytest.raises(AssertionError):       # bp_inference.py:179-189
        bp.update_bp_messages(c["S"].astype(np.float64), c["rvi"], c["rvc"], np.zeros_like(c["S"]))
    with pytest.raises(AssertionError):
        bp.update_bp_messages(c["S"], c["rvi"][:, :-1], c["rvc"], np.zeros_like(c["S"]))
    with pytest.raises(NotImplementedError):
        get_bp_backend("numpy", _GP(c["grid"], M))
    with pytest.raises(ValueError):
        get_bp_backend("hip", _GP(c["grid"], M))


# ------------------------------------------------------------------ a7
@pytest.mark.parametrize("case", sorted(CU))
@pytest.mark.parametrize("generic", [False, True])
def test_fused_k1_k2(torch, oracle_mod, case, generic, request):
    """perform_raynet_fp closures (K1, K2) vs the oracle's fused functions and vs the
    reference's CUDA device functions executed on the host."""
    from raynet_amd.hip_implementations.options import PathOptions
    from raynet_amd.hip_implementations.raynet_fp import perform_raynet_fp
    c = CU[case]
    o, feats, vg = make_case(oracle_mod, c)
    fp, de = perform_raynet_fp(o.M, o.D, o.N, o.F, o.H, o.W, o.padding, o.bbox, o.grid_shape,
                               "sample_in_bbox")
    hip_ctx(o).set_options(PathOptions(generic_sweep=generic))     # (set, not read from the environment)
    assert hip_ctx(o).get_options()["generic_sweep"] == generic
    request.addfinalizer(lambda: hip_ctx(o).set_options(PathOptions()))
    n = len(c["ray_idxs"])
    dev = "cuda"
    prior = o.prior(float(c["gamma"]))
    acc_in = torch.from_numpy(prior).to(dev)
    acc_out = torch.from_numpy(prior.copy()).to(dev)
    msgs = torch.zeros((n, o.M), device=dev)
    rvi = torch.zeros((n, o.M, 3), dtype=torch.int32, device=dev)
    rvc = torch.zeros((n,), dtype=torch.int32, device=dev)
    Sv = torch.zeros((n, o.M), device=dev)
    vg_d = torch.from_numpy(vg).to(dev)
    feats_d = torch.from_numpy(feats).to(dev)
    ret = fp(c["ray_idxs"], feats_d, c["P"], c["P_inv"], c["center"], vg_d, rvi, rvc, Sv, acc_in,
             msgs, acc_out)
    assert ret is msgs
    # oracle
    acc_o = prior.copy()
    msgs_o = np.zeros((n, o.M), np.float32)
    rvi_o, rvc_o, Sv_o = o.fused_bp(c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"], vg,
                                    prior, msgs_o, acc_o)
    assert np.array_equal(rvc.cpu().numpy(), rvc_o)
    assert np.array_equal(rvi.cpu().numpy(), rvi_o)                    # bit-exact index maps
    tolS = 2e-6 if (generic or o.F != 32) else 2e-5
    assert np.abs(Sv.cpu().numpy() - Sv_o).max() <= tolS
    m = msgs.cpu().numpy()
    assert np.all(np.abs(m - msgs_o) <= logit_tol(msgs_o) * (1 if generic else 8))
    assert np.all(np.abs(m - c["msgs"]) <= logit_tol(c["msgs"]) * (1 if generic else 8))
    assert np.abs(acc_out.cpu().numpy() - acc_o).max() <= 2e-4
    # K2 on the oracle's accumulator / messages (isolates K2)
    depth = torch.zeros((n,), device=dev)
    rvi.zero_(); rvc.zero_(); Sv.zero_()
    de(c["ray_idxs"], feats_d, c["P"], c["P_inv"], c["center"], vg_d, rvi, rvc, Sv,
       torch.from_numpy(acc_o).to(dev), torch.from_numpy(msgs_o).to(dev), depth)
    _, _, S_new_o, depth_o = o.fused_depth(c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"],
                                           vg, acc_o, msgs_o)
    S_new = Sv.cpu().numpy()      # K2 leaves the final distribution in S_voxel_space
    assert np.abs(S_new - S_new_o).max() <= 1e-5
    d = np.abs(depth.cpu().numpy() - depth_o)
    flips = d > 1e-4
    # a flip is legitimate only where the two best voxels are a near tie
    for r in np.where(flips)[0]:
        top = np.sort(S_new_o[r])[::-1]
        assert top[0] - top[1] <= 2e-5, (r, top[:2])
    assert flips.mean() <= 0.02


@pytest.mark.parametrize("case", ["wide", "aniso"])
def test_resident_scene_path_equals_fused(torch, oracle_mod, case):
    """rn_scene_prepare / rn_scene_bp_sweep / rn_scene_depth (packed voxel lists, resident
    clipped columns, per-copy accumulators) give what K1 / K2 give."""
    c = CU[case]
    o, feats, vg = make_case(oracle_mod, c)
    ctx = hip_ctx(o)
    dev = "cuda"
    ctx.set_voxel_grid(torch.from_numpy(vg).to(dev))
    n = len(c["ray_idxs"])
    ridx = ctx.dev(c["ray_idxs"])
    feats_d = torch.from_numpy(feats).to(dev)
    P, Pi, cc = ctx.dev(c["P"]), ctx.dev(c["P_inv"]), ctx.dev(c["center"])
    vox = torch.zeros((n, o.M), dtype=torch.int32, device=dev)
    rvc = torch.zeros((n,), dtype=torch.int32, device=dev)
    Sr = torch.zeros((n, o.M), device=dev)
    ctx.scene_prepare(ridx, [feats_d[v] for v in range(o.N)], P, Pi, cc, vox, rvc, Sr)
    rvi = c["rvi"].astype(np.int32)
    packed = (rvi[..., 0] << 20) | (rvi[..., 1] << 10) | rvi[..., 2]
    vox_h, rvc_h = vox.cpu().numpy(), rvc.cpu().numpy()
    assert np.array_equal(rvc_h, c["rvc"])
    for r in range(n):
        assert np.array_equal(vox_h[r, :rvc_h[r]], packed[r, :rvc_h[r]])
    prior_v = float(np.float32(np.log(0.05) - np.log(0.95)))
    # resident accumulators: flat, 4x4x4-bricked (rn_acc_size / rn_acc_to_grid / _from_grid)
    Gb = ctx.acc_size()
    assert Gb >= int(np.prod(o.grid_shape)) and Gb % 64 == 0
    acc_in = torch.full((Gb,), prior_v, device=dev)
    part = torch.zeros((ctx.acc_copies(), Gb), device=dev)
    acc_next = torch.empty((Gb,), device=dev)
    msgs = torch.zeros((n, o.M), device=dev)
    acc_o = o.prior(0.05)
    msgs_o = np.zeros((n, o.M), np.float32)
    for it in range(3):
        ctx.scene_bp_sweep(Sr, vox, rvc, acc_in, msgs, part)
        ctx.acc_combine(part, prior_v, acc_next)
        acc_in, acc_next = acc_next, acc_in
        assert float(part.abs().max()) == 0.0          # copies are re-zeroed
        out = o.prior(0.05)
        o.fused_bp(c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"], vg, acc_o, msgs_o, out)
        acc_o = out
    assert np.all(np.abs(msgs.cpu().numpy() - msgs_o) <= logit_tol(msgs_o) * 8)
    assert np.abs(ctx.acc_to_grid(acc_in).cpu().numpy() - acc_o).max() <= 5e-4
    # grid -> bricks -> grid is the identity
    assert np.array_equal(ctx.acc_to_grid(ctx.acc_from_grid(acc_o)).cpu().numpy(), acc_o)
    S_new = torch.zeros((n, o.M), device=dev)
    depth = torch.zeros((n,), device=dev)
    ctx.scene_depth(Sr, vox, rvc, ctx.acc_from_grid(acc_o), torch.from_numpy(msgs_o).to(dev),
                    cc, S_new, depth)
    _, _, S_new_o, depth_o = o.fused_depth(c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"],
                                           vg, acc_o, msgs_o)
    assert np.abs(S_new.cpu().numpy() - S_new_o).max() <= 1e-5
    # distributions within 1e-5 of each other: only a near-tie of <= 2e-5 can flip the arg-max
    assert assert_depth_flips_are_near_ties(depth.cpu().numpy(), depth_o, S_new_o, 2e-5,
                                            "resident K2") <= 0.02 * n


def test_sweep_order_changes_only_the_schedule(torch, oracle_mod):
    """rn_scene_prepare with a permutation `order` writes bit-identical columns."""
    c = CU["wide"]
    o, feats, vg = make_case(oracle_mod, c)
    ctx = hip_ctx(o)
    ctx.set_voxel_grid(torch.from_numpy(vg).cuda())
    n = len(c["ray_idxs"])
    ridx = ctx.dev(c["ray_idxs"])
    fv = [torch.from_numpy(feats).cuda()[v] for v in range(o.N)]
    P, Pi, cc = ctx.dev(c["P"]), ctx.dev(c["P_inv"]), ctx.dev(c["center"])
    outs = []
    for order in (None, torch.randperm(n, device="cuda").to(torch.int32)):
        vox = torch.zeros((n, o.M), dtype=torch.int32, device="cuda")
        rvc = torch.zeros((n,), dtype=torch.int32, device="cuda")
        Sr = torch.zeros((n, o.M), device="cuda")
        ctx.scene_prepare(ridx, fv, P, Pi, cc, vox, rvc, Sr, order=order)
        outs.append((vox.cpu().numpy(), rvc.cpu().numpy(), Sr.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


def test_config4_shapes_vs_oracle(torch, oracle_mod):
    """BASELINE.json config 4 shapes (9 views, 128 planes, M = 768 -> 12 register chunks,
    two plane chunks, the 9-view cooperative sweep) on a small image, against the oracle."""
    from raynet_amd.hip_implementations.raynet_fp import perform_raynet_fp
    from raynet_amd.synthetic import make_synthetic_scene
    H, W, D, M, N, grid = 20, 28, 128, 768, 9, (256, 256, 256)
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=N, focal=1.5 * H)
    o = oracle_mod.Oracle(M=M, D=D, N=N, F=32, H=H, W=W, padding=11, bbox=scene.bbox.ravel(),
                          grid_shape=grid, threads=oracle_mod.Oracle.max_threads())
    vg = oracle_mod.voxel_grid_centers(scene.bbox.ravel(), grid)
    views = scene.view_indices_with_neighbors(4, N - 1)
    assert len(views) == N
    feats = bank.stacked(views)
    P = np.array([scene.get_image(v).camera.P for v in views], np.float32)
    Pi = scene.get_image(4).camera.P_pinv.astype(np.float32)
    cc = scene.get_image(4).camera.center.ravel().astype(np.float32)
    n = H * W
    ridx = np.arange(n, dtype=np.int32)
    fp, de = perform_raynet_fp(M, D, N, 32, H, W, 11, scene.bbox.ravel(), grid, "sample_in_bbox")
    prior = o.prior(0.05)
    dev = "cuda"
    acc_out = torch.from_numpy(prior.copy()).to(dev)
    msgs = torch.zeros((n, M), device=dev)
    rvi = torch.zeros((n, M, 3), dtype=torch.int32, device=dev)
    rvc = torch.zeros((n,), dtype=torch.int32, device=dev)
    Sv = torch.zeros((n, M), device=dev)
    vg_d = torch.from_numpy(vg).to(dev)
    fp(ridx, feats, P, Pi, cc, vg_d, rvi, rvc, Sv, prior, msgs, acc_out)
    acc_o = prior.copy()
    msgs_o = np.zeros((n, M), np.float32)
    rvi_o, rvc_o, Sv_o = o.fused_bp(ridx, feats.cpu().numpy(), P, Pi, cc, vg, prior, msgs_o, acc_o)
    assert rvc_o.max() > 384                       # really exercises the long-ray chunks
    assert np.array_equal(rvc.cpu().numpy(), rvc_o)
    assert np.array_equal(rvi.cpu().numpy(), rvi_o)
    assert np.abs(Sv.cpu().numpy() - Sv_o).max() <= 2e-5
    m = msgs.cpu().numpy()
    assert np.all(np.abs(m - msgs_o) <= logit_tol(msgs_o) * 8)
    assert np.abs(acc_out.cpu().numpy() - acc_o).max() <= 5e-4
    depth = torch.zeros((n,), device=dev)
    de(ridx, feats, P, Pi, cc, vg_d, rvi, rvc, Sv, acc_o, msgs_o, depth)
    _, _, S_new_o, depth_o = o.fused_depth(ridx, feats.cpu().numpy(), P, Pi, cc, vg, acc_o, msgs_o)
    assert np.abs(Sv.cpu().numpy() - S_new_o).max() <= 1e-5
    assert assert_depth_flips_are_near_ties(depth.cpu().numpy(), depth_o, S_new_o, 2e-5,
                                            "config-4 K2") <= 0.02 * n


def test_mvcnn_kernels_k9_to_k12(torch, oracle_mod):
    from raynet_amd.hip_implementations.similarities import \
        perform_multi_view_cnn_forward_pass, \
        perform_multi_view_cnn_forward_pass_with_depth_estimation
    from raynet_amd.hip_implementations.mvcnn_with_ray_marching_and_voxels_mapping import \
        batch_mvcnn_voxel_traversal_with_ray_marching, \
        batch_mvcnn_voxel_traversal_with_ray_marching_with_depth_estimation
    c = CU["wide"]
    o, feats, vg = make_case(oracle_mod, c)
    n = len(c["ray_idxs"])
    args = (o.D, o.N, o.F, o.H, o.W, o.padding, o.bbox, "sample_in_bbox")
    S = torch.zeros((n, o.D), device="cuda")
    perform_multi_view_cnn_forward_pass(*args)(c["ray_idxs"], feats, c["P"], c["P_inv"],
                                               c["center"], S)
    assert np.abs(S.cpu().numpy() - c["S"]).max() <= 1e-5
    S2 = torch.zeros((n, o.D), device="cuda")
    pts = torch.zeros((n, o.D, 4), device="cuda")
    depth = torch.zeros((n,), device="cuda")
    perform_multi_view_cnn_forward_pass_with_depth_estimation(*args)(
        c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"], S2, pts, depth)
    k = np.argmax(c["S"], axis=1)                       # similarities.py:199-227
    p = pts.cpu().numpy()[np.arange(n), k, :3]
    expect = np.sqrt(((p - c["center"][:3]) ** 2).sum(1))
    near_tie = np.sort(c["S"], axis=1)[:, -1] - np.sort(c["S"], axis=1)[:, -2] < 1e-5
    assert np.abs(depth.cpu().numpy() - expect)[~near_tie].max() <= 1e-5
    vargs = (o.M, o.D, o.N, o.F, o.H, o.W, o.padding, o.bbox, o.grid_shape, "sample_in_bbox")
    rvi = torch.zeros((n, o.M, 3), dtype=torch.int32, device="cuda")
    rvc = torch.zeros((n,), dtype=torch.int32, device="cuda")
    Sv = torch.zeros((n, o.M), device="cuda")
    batch_mvcnn_voxel_traversal_with_ray_marching(*vargs)(
        c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"], vg, rvi, rvc, Sv)
    assert np.array_equal(rvi.cpu().numpy(), c["rvi"].astype(np.int32))
    assert np.abs(Sv.cpu().numpy() - c["S_voxel"]).max() <= 2e-5
    d12 = torch.zeros((n,), device="cuda")
    batch_mvcnn_voxel_traversal_with_ray_marching_with_depth_estimation(*vargs)(
        c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"], vg, rvi, rvc, Sv, d12)
    Svh = c["S_voxel"]
    i = np.argmax(Svh, axis=1)
    cen = vg[tuple(c["rvi"][np.arange(n), i].astype(np.int64).T)]
    expect = np.sqrt(((cen - c["center"][:3]) ** 2).sum(1))
    srt = np.sort(Svh, axis=1)
    near_tie = srt[:, -1] - srt[:, -2] < 1e-5
    assert np.abs(d12.cpu().numpy() - expect)[~near_tie].max() <= 1e-5


# ----------------------------------------------------------------- edges
def test_empty_and_state_errors(torch, oracle_mod):
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import HipContext
    ctx = HipContext(32, 8, 2, 4, 8, 8, 3, (0, 0, 0, 1, 1, 1), (4, 4, 4))
    z = torch.zeros((0, 3), device="cuda")
    ctx.voxel_traversal(z, z, torch.zeros((0, 32, 3), dtype=torch.int32, device="cuda"),
                        torch.zeros((0,), dtype=torch.int32, device="cuda"))       # n = 0 is fine
    with pytest.raises(_lib.RaynetHipError, match="RN_ERR_STATE"):
        ctx.planes_to_voxels(torch.zeros((1, 32, 3), dtype=torch.int32, device="cuda"),
                             torch.zeros((1,), dtype=torch.int32, device="cuda"),
                             torch.zeros((1, 3), device="cuda"), torch.zeros((1, 3), device="cuda"),
                             torch.zeros((1, 8), device="cuda"), torch.zeros((1, 32), device="cuda"))
    with pytest.raises(_lib.RaynetHipError):
        HipContext(32, 8, 2, 4, 8, 8, 3, (0, 0, 0, 1, 1, 1), (4, 4, 4000))      # grid too large
    from raynet_amd.ray_marching.ray_marching import get_voxel_traversal_backend
    from raynet_amd.forward_pass import get_forward_pass_factory
    with pytest.raises(NotImplementedError):
        get_voxel_traversal_backend("cython")
    with pytest.raises(KeyError):
        get_forward_pass_factory("hartmann_fp")


def test_rays_missing_the_box(torch, oracle_mod):
    """Rays that never enter the grid: count 0, no message, depth = distance to voxel
    (0,0,0) as in the reference's zero-filled buffers."""
    from raynet_amd.hip_implementations.raynet_fp import perform_raynet_fp
    c = CU["small"]
    o, feats, vg = make_case(oracle_mod, c)
    o2 = oracle_mod.Oracle(M=o.M, D=o.D, N=o.N, F=o.F, H=o.H, W=o.W, padding=o.padding,
                           bbox=(5, 5, 5, 6, 6, 6), grid_shape=o.grid_shape)
    vg2 = oracle_mod.voxel_grid_centers(o2.bbox, o2.grid_shape)
    fp, de = perform_raynet_fp(o.M, o.D, o.N, o.F, o.H, o.W, o.padding, o2.bbox, o2.grid_shape,
                               "sample_in_bbox")
    n = 64
    ridx = c["ray_idxs"][:n]
    prior = o2.prior(0.05)
    acc_out = torch.from_numpy(prior.copy()).cuda()
    msgs = torch.zeros((n, o.M), device="cuda")
    rvi = torch.zeros((n, o.M, 3), dtype=torch.int32, device="cuda")
    rvc = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    Sv = torch.zeros((n, o.M), device="cuda")
    fp(ridx, feats, c["P"], c["P_inv"], c["center"], vg2, rvi, rvc, Sv, prior, msgs, acc_out)
    assert int(rvc.abs().sum()) == 0 and float(msgs.abs().sum()) == 0.0
    assert np.array_equal(acc_out.cpu().numpy(), prior)
    depth = torch.zeros((n,), device="cuda")
    de(ridx, feats, c["P"], c["P_inv"], c["center"], vg2, rvi, rvc, Sv, prior, msgs, depth)
    expect = np.sqrt(((vg2[0, 0, 0] - c["center"][:3]) ** 2).sum())
    assert np.allclose(depth.cpu().numpy(), expect, rtol=1e-6)


@pytest.mark.parametrize("layout", ["linear", "patches", "shuffled"])
def test_box_scatter_equals_direct_sum(torch, oracle_mod, layout):
    """rn_scene_bp_sweep(row_layout=RN_ROWS_PATCHES) sums a tile's messages in an LDS image
    of its bounding box before touching the accumulator; whatever the row order (16x16
    patches = the fast case, ray-index order, a random shuffle = boxes that overflow LDS and
    fall back to direct atomics) the accumulator equals the float64 sum of the messages."""
    from raynet_amd.forward_pass import tile_order
    H, W, M, D, grid = 64, 48, 96, 16, (48, 48, 48)
    o = oracle_mod.Oracle(M=M, D=D, N=2, F=4, H=H, W=W, padding=3, bbox=[-1, -1, -1, 1, 1, 1],
                          grid_shape=grid)
    from raynet_amd.hip_implementations import get_context
    ctx = get_context(M, D, 2, 4, H, W, 3, [-1, -1, -1, 1, 1, 1], grid)
    vg = oracle_mod.voxel_grid_centers(np.array([-1, -1, -1, 1, 1, 1], np.float32), grid)
    ctx.set_voxel_grid(torch.from_numpy(vg).cuda())
    # a pinhole in front of the box: neighbouring pixels -> neighbouring rays
    n = H * W
    idx = torch.arange(n, dtype=torch.int32)
    if layout == "patches":
        idx = tile_order(idx, H, W, 16, 16)
    elif layout == "shuffled":
        idx = idx[torch.randperm(n, generator=torch.Generator().manual_seed(0))]
    x, y = (idx // H).numpy().astype(np.float32), (idx % H).numpy().astype(np.float32)
    cam = np.array([0.1, -0.2, -3.0], np.float32)
    tgt = np.stack([(x / W - 0.5) * 1.8, (y / H - 0.5) * 1.8, np.ones(n, np.float32)], 1)
    d = tgt - cam
    starts = (cam + d * (2.0 / d[:, 2:3])).astype(np.float32)       # plane z = -1
    ends = (cam + d * (4.0 / d[:, 2:3])).astype(np.float32)         # plane z = +1
    rvi, rvc = o.traversal(starts, ends)
    assert rvc.max() > 40 and rvc.max() <= M
    rng = np.random.default_rng(1)
    Sr = rng.random((n, M)).astype(np.float32) + 0.01
    Sr *= np.arange(M)[None, :] < rvc[:, None]
    Sr /= np.maximum(Sr.sum(1, keepdims=True), 1e-30)
    packed = ((rvi[..., 0] << 20) | (rvi[..., 1] << 10) | rvi[..., 2]).astype(np.int32)
    G = tuple(grid)
    prior_v = float(np.float32(np.log(0.05) - np.log(0.95)))
    acc_in = torch.full((ctx.acc_size(),), prior_v, device="cuda")
    outs = {}
    for patch_rows in (False, True):
        part = torch.zeros((ctx.acc_copies(), ctx.acc_size()), device="cuda")
        msgs = torch.zeros((n, M), device="cuda")
        ctx.scene_bp_sweep(torch.from_numpy(Sr).cuda(), torch.from_numpy(packed).cuda(),
                           torch.from_numpy(rvc).cuda(), acc_in, msgs, part, first_sweep=True,
                           patch_rows=patch_rows)
        outs[patch_rows] = (ctx.acc_to_grid(part.sum(0)).cpu().numpy(), msgs.cpu().numpy())
    assert np.array_equal(outs[False][1], outs[True][1])           # same k_bp, same messages
    m = outs[True][1].astype(np.float64)
    truth = np.zeros(G, np.float64)
    for r in range(n):
        c = int(rvc[r])
        if c > 1:
            np.add.at(truth, tuple(rvi[r, :c].T), m[r, :c])
    scale = np.abs(truth).max()
    assert np.abs(outs[True][0] - truth).max() < 2e-6 * scale
    assert np.abs(outs[False][0] - truth).max() < 2e-5 * scale
    # ... and the boxes do what the docstring says, by the kernel's own counters: a context of its
    # own per pinned tile shape, two sweeps with the device idle in between -- scatter_state()
    # then holds the first sweep's counters (tests/test_scatter_paths_gpu.py).  The census is the
    # host's count of the same thing.  (128 x 32 tiles: one chunk of the patches' 57 -- tile 6,
    # chunk 1, a box of 4158 voxels -- is above the 4096 of the LDS box; 256 x 16: none is.)
    from scatter_truth import census
    from raynet_amd.hip_implementations.context import HipContext
    from raynet_amd.hip_implementations.options import PathOptions
    Sr_d, packed_d, rvc_d = (torch.from_numpy(a).cuda() for a in (Sr, packed, rvc))
    for level in (0, 1):
        own = HipContext(M, D, 2, 4, H, W, 3, [-1, -1, -1, 1, 1, 1], grid)
        own.set_voxel_grid(torch.from_numpy(vg).cuda())
        own.set_options(PathOptions(box_level=level, box_pin=True))
        for sweep in range(2):
            part = torch.zeros((own.acc_size(),), device="cuda")
            own.scene_bp_sweep(Sr_d, packed_d, rvc_d, acc_in, torch.zeros((n, M), device="cuda"),
                               part, first_sweep=True, patch_rows=True)
            torch.cuda.synchronize()
        c = census(rvi, rvc, M, level)
        lv, chunks, overflowed = own.scatter_state()
        assert (lv, chunks, overflowed) == (level, c["chunks"], c["overflowed"])
        if layout == "shuffled":
            assert overflowed > 0 and c["nofit"] > 0
        elif layout == "patches" and level == 1:
            assert overflowed == 0


def test_box_scatter_with_caller_made_voxel_lists(torch, oracle_mod):
    """Voxel lists that are NOT a DDA walk (random, repeated voxels): elements outside the
    tile's end-point box take the direct-atomic route; sums stay exact."""
    M, D, grid = 32, 8, (15, 16, 18)          # not multiples of the 4x4x4 brick
    from raynet_amd.hip_implementations import get_context
    ctx = get_context(M, D, 2, 4, 8, 8, 3, [-1, -1, -1, 1, 1, 1], grid)
    vg = oracle_mod.voxel_grid_centers(np.array([-1, -1, -1, 1, 1, 1], np.float32), grid)
    ctx.set_voxel_grid(torch.from_numpy(vg).cuda())
    rng = np.random.default_rng(3)
    n = 700                                   # not a multiple of the tile
    rvi = np.stack([rng.integers(0, g, size=(n, M)) for g in grid], -1).astype(np.int32)
    rvi[:50] = rvi[0]                          # many rays through identical voxels
    rvc = rng.integers(0, M + 1, size=n).astype(np.int32)
    Sr = rng.random((n, M)).astype(np.float32) + 0.01
    Sr *= np.arange(M)[None, :] < rvc[:, None]
    Sr /= np.maximum(Sr.sum(1, keepdims=True), 1e-30)
    packed = ((rvi[..., 0] << 20) | (rvi[..., 1] << 10) | rvi[..., 2]).astype(np.int32)
    G = tuple(grid)
    acc_in = torch.full((ctx.acc_size(),), -2.9, device="cuda")
    part = torch.zeros((ctx.acc_copies(), ctx.acc_size()), device="cuda")
    msgs = torch.zeros((n, M), device="cuda")
    ctx.scene_bp_sweep(torch.from_numpy(Sr).cuda(), torch.from_numpy(packed).cuda(),
                       torch.from_numpy(rvc).cuda(), acc_in, msgs, part, first_sweep=True,
                       patch_rows=True)
    m = msgs.cpu().numpy().astype(np.float64)
    truth = np.zeros(G, np.float64)
    for r in range(n):
        c = int(rvc[r])
        if c > 1:
            np.add.at(truth, tuple(rvi[r, :c].T), m[r, :c])
    assert np.isfinite(m).all()
    got = ctx.acc_to_grid(part.sum(0)).cpu().numpy()
    assert np.abs(got - truth).max() < 1e-5 * max(1.0, np.abs(truth).max())


def test_maximum_sizes_m1024(torch, oracle_mod):
    """M = 1024 (the library's maximum: 16 register chunks) on a grid with a 1000-voxel axis,
    so that rays really have ~1000 voxels: K3 / K4 against the oracle; and the limits
    rn_create refuses."""
    from raynet_amd import _lib
    from raynet_amd.hip_implementations import get_context, HipContext
    M, D, grid = 1024, 8, (1000, 4, 4)
    bbox = np.array([-10, -0.04, -0.04, 10, 0.04, 0.04], np.float32)
    o = oracle_mod.Oracle(M=M, D=D, N=2, F=4, H=4, W=4, padding=3, bbox=bbox, grid_shape=grid)
    n = 70
    rng = np.random.default_rng(2)
    starts = np.c_[-10 * np.ones(n), rng.uniform(-0.03, 0.03, (n, 2))].astype(np.float32)
    ends = np.c_[10 * np.ones(n), rng.uniform(-0.03, 0.03, (n, 2))].astype(np.float32)
    ends[:10, 0] = rng.uniform(-9, 9, 10)             # some shorter rays
    rvi, rvc = o.traversal(starts, ends)
    assert rvc.max() >= 1000 and rvc.min() > 10
    S = rng.random((n, M)).astype(np.float32) + 0.01
    S *= np.arange(M)[None, :] < rvc[:, None]
    S /= S.sum(1, keepdims=True)
    ctx = get_context(M, D, 2, 4, 4, 4, 3, bbox, grid)
    dev = "cuda"
    rvi_d, rvc_d = torch.from_numpy(rvi).to(dev), torch.from_numpy(rvc).to(dev)
    prior = o.prior(0.05)
    acc_in = torch.from_numpy(prior).to(dev)
    acc_out = torch.from_numpy(prior.copy()).to(dev)
    msgs = torch.zeros((n, M), device=dev)
    ctx.bp_sweep(torch.from_numpy(S).to(dev), rvi_d, rvc_d, acc_in, msgs, acc_out, msgs)
    acc_o, msgs_o = prior.copy(), np.zeros((n, M), np.float32)
    o.bp_sweep(S, rvi, rvc, prior, msgs_o, acc_o)
    assert np.all(np.abs(msgs.cpu().numpy() - msgs_o) <= logit_tol(msgs_o) * 8)
    assert np.abs(acc_out.cpu().numpy() - acc_o).max() <= 1e-3
    S_new = torch.zeros((n, M), device=dev)
    ctx.depth_estimation(torch.from_numpy(S).to(dev), rvi_d, rvc_d, torch.from_numpy(acc_o).to(dev),
                         torch.from_numpy(msgs_o).to(dev), S_new)
    assert np.abs(S_new.cpu().numpy() - o.depth_distribution(S, rvi, rvc, acc_o, msgs_o)).max() <= 1e-5
    # limits: M > 1024, a grid axis > 1024, feature maps beyond 32-bit byte offsets
    for kw in (dict(M=1025), dict(grid_shape=(1025, 4, 4)), dict(H=20000, W=20000, F=32)):
        args = dict(M=8, D=8, N=2, F=4, H=4, W=4, padding=3, bbox=bbox, grid_shape=(4, 4, 4))
        args.update(kw)
        with pytest.raises(_lib.RaynetHipError):
            HipContext(**args)


def test_scatter_levels_agree_and_fixed_point_is_level_independent(torch, oracle_mod, monkeypatch):
    """The three scatter levels the launcher can choose (128x32 box, 256x16 box, slab /
    direct) produce the same accumulator -- to float-atomic tolerance in the default mode, and
    BIT-IDENTICAL in the fixed-point mode, whose integer sums do not depend on how the pairs
    are grouped."""
    from raynet_amd.forward_pass import tile_order
    from raynet_amd.hip_implementations.context import HipContext
    H, W, M, D, grid = 64, 48, 96, 16, (48, 48, 48)
    bbox = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    o = oracle_mod.Oracle(M=M, D=D, N=2, F=4, H=H, W=W, padding=3, bbox=bbox, grid_shape=grid)
    vg = oracle_mod.voxel_grid_centers(bbox, grid)
    n = H * W
    idx = tile_order(torch.arange(n, dtype=torch.int32), H, W, 16, 16)
    x, y = (idx // H).numpy().astype(np.float32), (idx % H).numpy().astype(np.float32)
    cam = np.array([0.1, -0.2, -3.0], np.float32)
    d = np.stack([(x / W - 0.5) * 1.8, (y / H - 0.5) * 1.8, np.ones(n, np.float32)], 1) - cam
    starts = (cam + d * (2.0 / d[:, 2:3])).astype(np.float32)
    ends = (cam + d * (4.0 / d[:, 2:3])).astype(np.float32)
    rvi, rvc = o.traversal(starts, ends)
    rng = np.random.default_rng(4)
    Sr = rng.random((n, M)).astype(np.float32) + 0.01
    Sr *= np.arange(M)[None, :] < rvc[:, None]
    Sr /= np.maximum(Sr.sum(1, keepdims=True), 1e-30)
    packed = torch.from_numpy(((rvi[..., 0] << 20) | (rvi[..., 1] << 10) | rvi[..., 2])
                              .astype(np.int32)).cuda()
    Sr_d, rvc_d = torch.from_numpy(Sr).cuda(), torch.from_numpy(rvc).cuda()
    monkeypatch.setenv("RAYNET_HIP_BOX_PIN", "1")
    floats, fixeds = [], []
    for level in (0, 1, 2):
        monkeypatch.setenv("RAYNET_HIP_BOX_LEVEL", str(level))
        ctx = HipContext(M, D, 2, 4, H, W, 3, bbox, grid)       # env is read at rn_create
        ctx.set_voxel_grid(torch.from_numpy(vg).cuda())
        G = ctx.acc_size()
        acc_in = torch.full((G,), -2.9, device="cuda")
        part = torch.zeros((1, G), device="cuda")
        msgs = torch.zeros((n, M), device="cuda")
        ctx.scene_bp_sweep(Sr_d, packed, rvc_d, acc_in, msgs, part, first_sweep=True,
                           patch_rows=True)
        floats.append(ctx.acc_to_grid(part[0]).cpu().numpy())
        part64 = torch.zeros((G,), dtype=torch.int64, device="cuda")
        ctx.scene_bp_sweep_fixed(Sr_d, packed, rvc_d, acc_in, msgs, part64, first_sweep=True,
                                 patch_rows=True)
        out = torch.empty((G,), device="cuda")
        ctx.acc_combine_fixed(part64, 0.0, out)
        assert int(part64.abs().max()) == 0                      # partial zeroed by the combine
        fixeds.append(ctx.acc_to_grid(out).cpu().numpy())
    scale = np.abs(floats[0]).max()
    assert scale > 1.0
    for level in (1, 2):
        assert np.abs(floats[level] - floats[0]).max() < 2e-5 * scale
        assert np.array_equal(fixeds[level], fixeds[0])
    assert np.abs(fixeds[0] - floats[0]).max() < 2e-5 * scale


def test_exact_arithmetic_shortcuts(torch, oracle_mod):
    """round_half_away (3 instructions) == roundf bit for bit on the GPU: 4 M random bit
    patterns plus the half-way edges.  (tools/verify_round_trick.c walks all 2^32 floats on
    the CPU.)"""
    o, _, _ = make_case(oracle_mod, CU["small"])
    ctx = hip_ctx(o)
    rng = np.random.default_rng(5)
    n = 1 << 22
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    k = np.arange(4096, dtype=np.float32)
    edges = np.concatenate([k + 0.5, -(k + 0.5), np.nextafter(k + 0.5, 0).astype(np.float32),
                            np.nextafter(k + 0.5, 1e9).astype(np.float32), k, -k,
                            np.float32(2.0) ** np.arange(-45, 40, dtype=np.float32),
                            np.float32(2.0) ** 23 + k, np.float32(2.0) ** 22 + k + 0.5])
    a[:edges.size] = edges
    out = torch.zeros((2, n), device="cuda")
    ctx.selftest_arith(torch.from_numpy(a).cuda(), out)
    out = out.cpu().numpy()
    ok = np.isnan(a) | (out[0].view(np.uint32) == out[1].view(np.uint32))
    assert ok.all(), "round_half_away differs from roundf"
    with np.errstate(all="ignore"):
        expect = np.where(np.isfinite(a), np.trunc(a.astype(np.float64) + np.copysign(0.5, a)), a)
    fin = np.isfinite(a)
    assert np.array_equal(out[0][fin], expect.astype(np.float32)[fin])


def test_stitch_rows_into_device_and_pinned_host_memory(torch, oracle_mod):
    """rn_stitch_rows: out[i] = rows[index[i]] -- the ranks' gathered depth rows into pixel order,
    written by the kernel into a CUDA tensor or straight into page-locked HOST memory (stitch and
    device-to-host copy in one launch); lengths that are not multiples of 4, an empty call,
    and the argument checks."""
    o, _, _ = make_case(oracle_mod, CU["small"])
    ctx = hip_ctx(o)
    rng = np.random.default_rng(11)
    for n, m in ((307200, 8 * 38912 + 1), (2745, 3001), (4, 4), (3, 9), (0, 5)):
        rows = torch.from_numpy(rng.standard_normal(m).astype(np.float32)).cuda()
        index = torch.from_numpy(rng.integers(0, m, n).astype(np.int32)).cuda()
        want = rows[index.long()].cpu().numpy()
        dev = torch.full((n + 8,), -7.0, device="cuda")
        ctx.stitch_rows(rows, index, dev)
        got = dev.cpu().numpy()
        assert np.array_equal(got[:n], want) and np.all(got[n:] == -7.0)
        host = torch.full((n + 8,), -7.0).pin_memory()
        ctx.stitch_rows(rows, index, host)
        torch.cuda.synchronize()
        assert np.array_equal(host.numpy()[:n], want) and np.all(host.numpy()[n:] == -7.0)
    rows = torch.zeros(16, device="cuda")
    index = torch.zeros(8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ctx.stitch_rows(rows, index, torch.zeros(8))                     # pageable host memory
    with pytest.raises(ValueError):
        ctx.stitch_rows(rows, index, torch.zeros(16, device="cuda")[1:])  # not 16-byte aligned
    with pytest.raises(ValueError):
        ctx.stitch_rows(rows, index.long(), torch.zeros(8, device="cuda"))


@pytest.mark.parametrize("D", [2, 3, 16, 64, 128, 1000, 4096])
def test_mapping_shortcuts_are_exact(torch, D):
    """The resident path's planes -> voxels mapping replaces (a) the division by |ray|^2 with
    Markstein's correctly rounded quotient from one IEEE reciprocal per ray and (b) the plane
    walk with a look-up in the table of the walk's own fp32 positions.  Bit for bit / index for
    index against the expressions they replace: quotients of ordinary magnitudes, of the
    extremes the range guard admits, and random bit patterns (where the guard is off, the
    kernels divide); t planted within a few ulps of every plane position, random t, the
    clamps' ends -- for plane counts from 2 to the 4096 rn_create admits."""
    from raynet_amd.hip_implementations import get_context
    ctx = get_context(M=64, D=D, N=2, F=4, H=8, W=8, padding=3, bbox=(0, 0, 0, 1, 1, 1),
                      grid_shape=(4, 4, 4))
    rng = np.random.default_rng(100 + D)
    n = 1 << 21
    q = n // 4
    a = np.empty(n, np.float32)
    b = np.empty(n, np.float32)
    # (a) what the mapping divides: sums of a few products over |ray|^2, any sign
    b[:q] = rng.uniform(1e-3, 50.0, q).astype(np.float32)
    a[:q] = (rng.uniform(-1.5, 2.5, q) * b[:q]).astype(np.float32)
    # (b) quotients next to representable results: a = RN(k * ulp-ish * b) nudged by +-2 ulps
    b[q:2 * q] = rng.uniform(0.01, 20.0, q).astype(np.float32)
    tq = rng.uniform(1e-4, 1.0, q).astype(np.float32)
    aa = (tq * b[q:2 * q]).astype(np.float32)
    a[q:2 * q] = (aa.view(np.int32) + rng.integers(-2, 3, q).astype(np.int32)).view(np.float32)
    # (c) the guard's extremes: divisors 2^-60 .. 2^60, dividends down to where the clamp hides them
    e = rng.integers(-60, 58, q)
    b[2 * q:3 * q] = np.ldexp(rng.uniform(1.0, 2.0, q), e).astype(np.float32)
    a[2 * q:3 * q] = (np.ldexp(rng.uniform(1.0, 2.0, q), e + rng.integers(-14, 2, q)) *
                      rng.choice([-1.0, 1.0], q)).astype(np.float32)
    # (d) anything
    a[3 * q:] = rng.integers(0, 1 << 32, q, dtype=np.uint64).astype(np.uint32).view(np.float32)
    b[3 * q:] = rng.integers(0, 1 << 32, q, dtype=np.uint64).astype(np.uint32).view(np.float32)
    # t: every plane position of this D moved by -3 .. 3 ulps, the clamps, random
    step = np.float32(1.0) / np.float32(D - 1)
    pos = (np.float32(0.0) + np.arange(D + 1, dtype=np.float32) * step).astype(np.float32)
    t = rng.uniform(0.0, 1.0, n).astype(np.float32)
    planted = (np.repeat(pos, 7).view(np.int32) + np.tile(np.arange(-3, 4, dtype=np.int32), D + 1))
    planted = planted.view(np.float32)[:n // 2]
    t[:planted.size] = planted
    t[planted.size:planted.size + 8] = [0.0, 1e-4, 1.0, 1 - 1e-4, 2.0, -1.0, 9.9e-5, 0.99995]
    # what the clamp (one v_med3_f32 for min(max(t, eps), 1 - eps)) does with values no ray
    # produces: NaN of either sign and payload -> eps like fmaxf, infinities, zeros, denormals
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 3e38,
                        -3e38, 0.5], np.float32)
    special[1] = np.uint32(0xffc00001).view(np.float32)
    # (quiet NaNs only: every clamped value of the path is the result of an arithmetic
    # instruction, which quiets a signalling NaN; v_med3_f32 would pass one on as 1 - eps)
    t[-special.size:] = special
    out = torch.zeros((5, n), device="cuda")
    ctx.selftest_mapping(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(),
                         torch.from_numpy(t).cuda(), out)
    exact, fast, ok, walk, table = out.cpu().numpy()
    ok = ok > 0
    assert ok[:3 * q].all()                         # everything a real ray produces is inside
    same = (exact.view(np.uint32) == fast.view(np.uint32)) | (np.isnan(exact) & np.isnan(fast))
    # where the result is clamped to eps anyway (|q| < 5e-5) a last-bit difference in the
    # denormal range is invisible; everywhere else the two are the same bits
    visible = np.abs(exact) >= 5e-5
    bad = np.flatnonzero(ok & visible & ~same)
    assert bad.size == 0, ("Markstein's quotient differs from the division", a[bad[:8]], b[bad[:8]],
                           exact[bad[:8]], fast[bad[:8]])
    with np.errstate(all="ignore"):
        host = a / b
    fin = np.isfinite(host)
    assert np.array_equal(exact[fin], host[fin])    # the GPU's division is the host's (IEEE)
    bad = np.flatnonzero(walk != table)
    assert bad.size == 0, ("table look-up differs from the walk", t[bad[:8]], walk[bad[:8]],
                           table[bad[:8]])
    tc = np.clip(t, np.float32(1e-4), np.float32(1 - 1e-4))
    expect = (pos[None, 1:D] < tc[:4096, None]).sum(1)          # #{l >= 1 : pos[l] < t}
    assert np.array_equal(walk[:4096].astype(np.int64), expect)
    with np.errstate(all="ignore"):
        tcs = np.where(np.isnan(special), np.float32(1e-4),
                       np.clip(special, np.float32(1e-4), np.float32(1 - 1e-4))).astype(np.float32)
    expect = (pos[None, 1:D] < tcs[:, None]).sum(1)
    assert np.array_equal(walk[-special.size:].astype(np.int64), expect), (walk[-special.size:], expect)
    assert np.array_equal(table[-special.size:].astype(np.int64), expect)


def test_rounded_quotient_shortcut(torch, oracle_mod):
    """round_quotient_fast (x * rcp(d), rounded) == roundf(x / d) bit for bit wherever it says
    it is sure: quotients planted within a few ulps of every rounding boundary k + 1/2 of a
    feature map's extent (where it must NOT be sure when the two could differ), ordinary
    projections, and random bit patterns (infinities, NaNs, denormals, zero divisors)."""
    o, _, _ = make_case(oracle_mod, CU["small"])
    ctx = hip_ctx(o)
    rng = np.random.default_rng(11)
    n = 1 << 22
    x = np.empty(n, np.float32)
    d = np.empty(n, np.float32)
    q = n // 4
    # (a) next to the boundaries: x = RN((k + 1/2) * d) moved by -3 .. 3 ulps
    dd = (rng.uniform(0.05, 40.0, q) * rng.choice([-1.0, 1.0], q)).astype(np.float32)
    k = rng.integers(-64, 4096, q).astype(np.float32)
    xx = ((k + np.float32(0.5)) * dd).astype(np.float32)
    xx = (xx.view(np.int32) + rng.integers(-3, 4, q).astype(np.int32)).view(np.float32)
    x[:q], d[:q] = xx, dd
    # (b) the same with exactly representable half-way quotients (d a power of two)
    dd = (np.float32(2.0) ** rng.integers(-6, 6, q).astype(np.float32)).astype(np.float32)
    x[q:2 * q], d[q:2 * q] = ((k + np.float32(0.5)) * dd).astype(np.float32), dd
    # (c) ordinary projections: pixel coordinates anywhere near an image, depths 0.1 .. 30
    dd = rng.uniform(0.1, 30.0, q).astype(np.float32)
    x[2 * q:3 * q], d[2 * q:3 * q] = (rng.uniform(-300.0, 2500.0, q) * dd).astype(np.float32), dd
    # (d) anything
    x[3 * q:] = rng.integers(0, 1 << 32, q, dtype=np.uint64).astype(np.uint32).view(np.float32)
    d[3 * q:] = rng.integers(0, 1 << 32, q, dtype=np.uint64).astype(np.uint32).view(np.float32)
    out = torch.zeros((3, n), device="cuda")
    ctx.selftest_quotient(torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda(), out)
    exact, fast, sure = out.cpu().numpy()
    sure = sure > 0
    same = exact.view(np.uint32) == fast.view(np.uint32)
    bad = np.flatnonzero(sure & ~same)
    assert bad.size == 0, ("round_quotient_fast is sure of a value the division does not give",
                           x[bad[:8]], d[bad[:8]], exact[bad[:8]], fast[bad[:8]])
    # the division agrees with the host's, so `exact` is the reference's arithmetic
    with np.errstate(all="ignore"):
        host = x / d
        fin = np.isfinite(host) & (np.abs(host) < 2.0 ** 22)
        expect = np.trunc(host.astype(np.float64) + np.copysign(0.5, host))
    assert np.array_equal(exact[fin], expect[fin].astype(np.float32))
    # it is sure of nearly all ordinary projections (the fallback stays rare) and of nothing
    # that is not finite
    assert sure[2 * q:3 * q].mean() > 0.995
    assert not sure[~np.isfinite(fast)].any()
    assert not sure[q:2 * q].any()          # exact half-way cases are never "sure"
