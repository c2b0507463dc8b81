"""The MRF training kernels of csrc/raynet_train.inl held PER LAUNCH to float64, at rows of one,
two, three and sixteen chunks of 64: k_ray_bwd<0> (train_bp_sweep_bwd), k_ray_bwd<1>
(train_depth_bwd) and the unclipped-input forwards (train_bp_sweep, train_depth), called through
HipContext directly.  Truths, inputs and the E_* constants: tests/mrf_bwd_truth.py; each
tolerance is GPU_FACTOR (16) x the error the sequential fp32 restatement of the same formulas
has on these inputs (tests/test_mrf_bwd_truth.py), never a figure the kernel returned."""
import numpy as np
import pytest

import mrf_bwd_truth as mt

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENTINEL = 7.0
LN_CLAMP = float(np.log(9999.0))


@pytest.fixture(scope="module")
def contexts():
    """One training context per M on the 16^3 grid (M = 1024: the library's longest row, 14 LDS
    rows of 1024 floats per wavefront in k_ray_bwd)."""
    from raynet_amd.mrf import mrf_train
    bbox = np.array([-1, -1, -1, 1, 1, 1], np.float32)
    axes = [np.linspace(-1, 1, g + 1)[:-1] + 1.0 / g for g in mt.GRID]
    vg = np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(np.float32)
    return {M: mrf_train.training_context(M, 8, bbox, mt.GRID, vg) for M in mt.GPU_COUNTS}


def _dev(p):
    import torch
    d = {k: torch.from_numpy(p[k]).cuda() for k in ("Sr", "rvi", "rvc", "msgs", "g_out")}
    d["acc"] = torch.from_numpy(p["acc"].ravel()).cuda()
    d["g_acc_out"] = torch.from_numpy(p["g_acc_out"].ravel()).cuda()
    return d


def _launch_bwd(hip, d, mode, old_s=0.0, old_acc=0.0, old_msgs=0.0):
    """One backward launch into buffers pre-filled with the given values -> numpy (g_s, g_acc, g_msgs)."""
    import torch
    g_s = torch.full_like(d["Sr"], old_s)
    g_acc = torch.full_like(d["acc"], old_acc)
    g_msgs = torch.full_like(d["Sr"], old_msgs)
    if mode == 0:
        hip.train_bp_sweep_bwd(d["Sr"], d["rvi"], d["rvc"], d["acc"], d["msgs"], d["g_out"],
                               d["g_acc_out"], g_s, g_acc, g_msgs)
    else:
        hip.train_depth_bwd(d["Sr"], d["rvi"], d["rvc"], d["acc"], d["msgs"], d["g_out"], g_s,
                            g_acc, g_msgs)
    torch.cuda.synchronize()
    return g_s.cpu().numpy(), g_acc.cpu().numpy().reshape(mt.GRID), g_msgs.cpu().numpy()


def _tol(mode, output, regime):
    tol = mt.GPU_FACTOR * mt.E(mt.MODES[mode], output, regime)
    assert 0 < tol <= 1e-3          # half the chain tolerance: beyond it the INPUTS are wrong
    return tol


def _check_rows(mode, output, regime, got, ref, rvc, slack=None):
    """got [n, M] against ref below each count: per ray on the ray's own largest |ref| (per launch
    for the one combination of mrf_bwd_truth.LAUNCH_WIDE).  slack [n, M]: absolute rounding of
    what the test itself added on top (the pre-filled value).  Returns the worst err / bound."""
    tol = _tol(mode, output, regime)
    wide = (mt.MODES[mode], output, regime) in mt.LAUNCH_WIDE
    worst = 0.0
    for r in range(len(rvc)):
        c = int(rvc[r])
        if c <= 1:
            continue
        scale = np.abs(ref).max() if wide else np.abs(ref[r, :c]).max()
        err = np.abs(got[r, :c] - ref[r, :c])
        bound = tol * scale + (0.0 if slack is None else slack[r, :c])
        ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
        assert ratio <= 1, "%s %s %s: ray %d (count %d) err %g, bound %g (ratio %g)" % (
            mt.MODES[mode], output, regime, r, c, err.max(), np.max(bound), ratio)
        worst = max(worst, ratio)
    return worst


def _check_acc(mode, regime, got, ref, slack=0.0):
    tol = _tol(mode, "gacc", regime)
    err = np.abs(got - ref)
    ratio = float((err / (tol * np.abs(ref).max() + slack)).max())
    assert ratio <= 1, "%s gacc %s: err %g, ratio %g" % (mt.MODES[mode], regime, err.max(), ratio)
    return ratio


# ------------------------------------------------------------------ a. values
@pytest.mark.parametrize("regime", mt.REGIMES)
@pytest.mark.parametrize("mode", [0, 1], ids=mt.MODES)
@pytest.mark.parametrize("M", sorted(mt.GPU_COUNTS))
def test_backward_launch_against_float64(contexts, M, mode, regime):
    p = mt.gpu_launch(M, regime)
    ref_s, ref_acc, ref_msgs = mt.gpu_truth(M, regime, mode)
    g_s, g_acc, g_msgs = _launch_bwd(contexts[M], _dev(p), mode)
    assert np.isfinite(g_s).all() and np.isfinite(g_acc).all() and np.isfinite(g_msgs).all()
    ratios = (_check_rows(mode, "gs", regime, g_s, ref_s, p["rvc"]),
              _check_rows(mode, "gmsgs", regime, g_msgs, ref_msgs, p["rvc"]),
              _check_acc(mode, regime, g_acc, ref_acc))
    print("worst err / bound (g_s, g_msgs, g_acc), M %d %s %s: %.3f %.3f %.3f"
          % ((M, mt.MODES[mode], regime) + ratios))


# ------------------------------------------------------------------ b. the output contract
@pytest.mark.parametrize("regime", ["prior", "saturated"])
@pytest.mark.parametrize("mode", [0, 1], ids=mt.MODES)
def test_backward_output_contract(contexts, mode, regime):
    """g_s and g_acc ACCUMULATE into what is there, g_msgs is ASSIGNED below the count and left
    alone at and beyond it; a skipped ray (count <= 1) adds nothing and writes zeros below its
    count.  mrf_train.MRFDepthDistribution.backward relies on each of these."""
    M = 192
    p = mt.gpu_launch(M, regime)
    rvc, rvi = p["rvc"], p["rvi"]
    ref_s, ref_acc, ref_msgs = mt.gpu_truth(M, regime, mode)
    old_s, old_acc = 0.5, -0.25
    g_s, g_acc, g_msgs = _launch_bwd(contexts[M], _dev(p), mode, old_s, old_acc, SENTINEL)
    below = np.arange(M)[None, :] < rvc[:, None]
    live = below & (rvc > 1)[:, None]
    # untouched: everything of g_s outside the live entries, g_msgs at and beyond the count,
    # g_acc at voxels no live entry names
    assert np.all(g_s[~live] == np.float32(old_s))
    assert np.all(g_msgs[~below] == np.float32(SENTINEL))
    assert np.all(g_msgs[below & ~live] == 0)                     # count 1: a zero at entry 0
    touched = np.zeros(mt.GRID, bool)
    touched[tuple(rvi[live].T)] = True
    assert touched.any() and not touched.all() and np.all(g_acc[~touched] == np.float32(old_acc))
    # old + truth, to the launch's tolerance plus the rounding of the additions themselves:
    # one fp32 addition for g_s, one per contributing ray for g_acc (each within half an ulp
    # of at most |old| + sum |contribution|)
    _check_rows(mode, "gs", regime, g_s, ref_s + old_s * live, rvc,
                slack=EPS * (abs(old_s) + np.abs(ref_s)))
    _check_rows(mode, "gmsgs", regime, g_msgs, ref_msgs, rvc)
    adds = np.zeros(mt.GRID)
    mass = np.zeros(mt.GRID)
    np.add.at(adds, tuple(rvi[live].T), 1.0)
    np.add.at(mass, tuple(rvi[live].T), np.abs(ref_msgs[live]))    # |dL/dmu| of each entry
    got = np.where(touched, g_acc, 0.0)
    want = np.where(touched, ref_acc + old_acc, 0.0)
    err = np.abs(got - want)
    bound = _tol(mode, "gacc", regime) * np.abs(ref_acc).max() + EPS * adds * (abs(old_acc) + mass)
    assert np.all(err <= bound), (err.max(), float((err / np.maximum(bound, 1e-300)).max()))


# ------------------------------------------------------------------ c. the training forwards
@pytest.mark.parametrize("regime", mt.REGIMES)
@pytest.mark.parametrize("M", sorted(mt.GPU_COUNTS))
def test_forward_launches_against_float64(contexts, M, regime):
    """launch_bp<false, false> / launch_depth<false, false> (no clip inside: nothing else uses
    them) at long rows.  Messages: the bound of test_bp_single_sweep_against_float64_truth
    (tests/test_hip_parity_gpu.py); the accumulator: the float64 scatter of the returned
    messages, as there; the distribution: the 5e-5 of the chain tests."""
    import torch
    hip, p = contexts[M], mt.gpu_launch(M, regime)
    d = _dev(p)
    rvc, rvi = p["rvc"], p["rvi"]
    live = (np.arange(M)[None, :] < rvc[:, None]) & (rvc > 1)[:, None]
    base = -2.9444
    acc_out = torch.full_like(d["acc"], base)
    m_out = torch.zeros_like(d["Sr"])
    hip.train_bp_sweep(d["Sr"], d["rvi"], d["rvc"], d["acc"], d["msgs"], acc_out, m_out)
    dist = torch.zeros_like(d["Sr"])
    hip.train_depth(d["Sr"], d["rvi"], d["rvc"], d["acc"], d["msgs"], dist)
    torch.cuda.synchronize()
    m_out, acc_out, dist = m_out.cpu().numpy(), acc_out.cpu().numpy().reshape(mt.GRID), dist.cpu().numpy()
    truth, _ = mt.sweep_fwd(p["Sr"], rvi, rvc, p["acc"], p["msgs"])
    assert np.isfinite(m_out).all() and not m_out[~live].any()
    cond = 2 + np.exp(np.minimum(np.abs(truth), 30))
    ratio = np.where(live, np.abs(m_out - truth) / (1e-3 + 32 * EPS * cond), 0)
    assert ratio.max() <= 1, (np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
    ref_acc = np.full(mt.GRID, np.float64(np.float32(base)))
    np.add.at(ref_acc, tuple(rvi[live].T), m_out[live].astype(np.float64))
    assert np.abs(acc_out - ref_acc).max() <= 1e-3
    ref_dist = mt.depth_fwd(p["Sr"], rvi, rvc, p["acc"], p["msgs"])
    assert np.abs(dist - ref_dist).max() < 5e-5 and not dist[~live].any()
    assert np.abs(dist[rvc > 1].sum(1, dtype=np.float64) - 1).max() < 1e-5


# ------------------------------------------------------------------ d. launches chained
def test_two_sweep_composition_at_the_kernel_level(contexts):
    """Depth backward, then the sweep backward over the stored state of sweep 1, then of sweep 0,
    chained as MRFDepthDistribution.backward chains them (g_msgs -> g_msgs_out, g_acc ->
    g_acc_out, g_s accumulating), against the same chain of the launch truths on the SAME stored
    fp32 states: the plumbing between launches, without the mapping and the clip in front.
    Bound: every launch contributes at most its own 16 x E (the largest over its outputs) of the
    launch-wide scale, and the backward is linear in the incoming gradient."""
    import torch
    M, regime = 192, "prior"
    hip, p = contexts[M], mt.gpu_launch(M, regime)
    d = _dev(p)
    rvi, rvc = p["rvi"], p["rvc"]
    accs, msgs = [d["acc"]], [d["msgs"]]
    for _ in range(2):
        acc_out = torch.full_like(d["acc"], -2.9444)
        m_out = torch.zeros_like(d["Sr"])
        hip.train_bp_sweep(d["Sr"], d["rvi"], d["rvc"], accs[-1], msgs[-1], acc_out, m_out)
        accs.append(acc_out)
        msgs.append(m_out)
    g_s = torch.zeros_like(d["Sr"])
    g_acc = torch.zeros_like(d["acc"])
    g_m = torch.zeros_like(d["Sr"])
    hip.train_depth_bwd(d["Sr"], d["rvi"], d["rvc"], accs[2], msgs[2], d["g_out"], g_s, g_acc, g_m)
    for it in (1, 0):
        g_acc_prev, g_m_prev = torch.zeros_like(g_acc), torch.zeros_like(g_m)
        hip.train_bp_sweep_bwd(d["Sr"], d["rvi"], d["rvc"], accs[it], msgs[it], g_m, g_acc, g_s,
                               g_acc_prev, g_m_prev)
        g_acc, g_m = g_acc_prev, g_m_prev
    torch.cuda.synchronize()
    A = [a.cpu().numpy().reshape(mt.GRID) for a in accs]
    Ms = [m.cpu().numpy() for m in msgs]
    # a condition on the inputs: the stored states are the kernels' own, not crafted ones, and
    # none of them sits where fp32 and float64 could disagree about the occupancy clamp
    live = (np.arange(M)[None, :] < rvc[:, None]) & (rvc > 1)[:, None]
    for a, m in zip(A, Ms):
        mu = a[tuple(rvi[live].T)].astype(np.float64) - m[live]
        assert np.abs(np.abs(mu) - LN_CLAMP).min() > 1e-3
    r_s, r_acc, r_m = mt.depth_bwd(p["Sr"], rvi, rvc, A[2], Ms[2], p["g_out"])
    for it in (1, 0):
        d_s, r_acc, r_m = mt.sweep_bwd(p["Sr"], rvi, rvc, A[it], Ms[it], r_m, r_acc)
        r_s = r_s + d_s
    tol = mt.GPU_FACTOR * (max(mt.E("depth", o, regime) for o in mt.OUTPUTS) +
                           2 * max(mt.E("sweep", o, regime) for o in mt.OUTPUTS))
    assert tol <= 1e-3
    for name, got, ref in (("g_s", g_s, r_s), ("g_acc", g_acc, r_acc), ("g_msgs", g_m, r_m)):
        got = got.cpu().numpy().reshape(ref.shape)
        scale = np.abs(ref).max()
        err = np.abs(got - ref).max()
        print("chain %s: err / (tol * scale) = %.3f" % (name, err / (tol * scale)))
        assert scale > 0 and err <= tol * scale, (name, err, scale)
