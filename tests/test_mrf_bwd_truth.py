"""CPU part of the per-launch checks of the MRF training kernels: the float64 launch truths of
tests/mrf_bwd_truth.py against central finite differences of their own forwards, the error of
the sequential fp32 restatement of k_ray_bwd against those truths (the E_* constants the GPU
tolerances of tests/test_mrf_backward_kernels_gpu.py are derived from), and the conditions the
crafted inputs meet."""
import numpy as np
import pytest

import mrf_bwd_truth as mt

FD_COUNTS = [2, 3, 65, 130, 0, 1, 65, 130, 3, 2]
FD_SAMPLES = 16          # coordinates per differentiated input (Sr, acc, msgs): 48 per case


def _fd_check(p, loss, grads, rng):
    """Central differences of `loss` at FD_SAMPLES used coordinates of each of Sr, acc and msgs,
    with the relative bound tests/test_mrf_backward.py holds the whole chain to.  The forward is
    evaluated in long double: behind a few dozen voxels of a long row the gradients fall below
    1e-6, where the rounding of a float64 loss of order 100, divided by 2h, is no longer small
    against the bound's floor."""
    assert np.finfo(np.longdouble).eps < 1e-18
    p = dict(p, **{k: p[k].astype(np.longdouble) for k in ("Sr", "acc", "msgs")})
    rvi, rvc = p["rvi"], p["rvc"]
    used = np.arange(rvi.shape[1])[None, :] < np.where(rvc > 1, rvc, 0)[:, None]
    vox = np.zeros(p["grid"], bool)
    for r in np.nonzero(rvc > 1)[0]:
        vox[tuple(rvi[r, :rvc[r]].T)] = True
    h = 1e-6
    worst, checked = 0.0, 0
    for name, mask in (("Sr", used), ("acc", vox), ("msgs", used)):
        where = np.argwhere(mask)
        for k in where[rng.choice(len(where), FD_SAMPLES, replace=False)]:
            k = tuple(k)
            hi, lo = dict(p), dict(p)
            for d, step in ((hi, h), (lo, -h)):
                d[name] = p[name].copy()
                d[name][k] += step
            fd = float((loss(hi) - loss(lo)) / (2 * h))
            an = grads[name][k]
            worst = max(worst, abs(fd - an) / max(1e-6, abs(fd), abs(an)))
            checked += 1
    assert checked == 3 * FD_SAMPLES and worst < 1e-4, worst


@pytest.mark.parametrize("regime", mt.REGIMES)
def test_sweep_bwd_matches_finite_differences(regime):
    p = mt.make_launch(FD_COUNTS, 130, regime, seed=11)
    gm, ga = p["g_out"].astype(np.float64), p["g_acc_out"].astype(np.float64)

    def loss(q):
        m, a = mt.sweep_fwd(q["Sr"], q["rvi"], q["rvc"], q["acc"], q["msgs"])
        return (gm * m).sum() + (ga * a).sum()

    g_s, g_acc, g_msgs = mt.sweep_bwd(p["Sr"], p["rvi"], p["rvc"], p["acc"], p["msgs"], gm, ga)
    skipped = p["rvc"] <= 1
    assert not g_s[skipped].any() and not g_msgs[skipped].any()
    _fd_check(p, loss, dict(Sr=g_s, acc=g_acc, msgs=g_msgs), np.random.default_rng(1))


@pytest.mark.parametrize("regime", mt.REGIMES)
def test_depth_bwd_matches_finite_differences(regime):
    p = mt.make_launch(FD_COUNTS, 130, regime, seed=12)
    g = p["g_out"].astype(np.float64)

    def loss(q):
        return (g * mt.depth_fwd(q["Sr"], q["rvi"], q["rvc"], q["acc"], q["msgs"])).sum()

    g_s, g_acc, g_msgs = mt.depth_bwd(p["Sr"], p["rvi"], p["rvc"], p["acc"], p["msgs"], g)
    _fd_check(p, loss, dict(Sr=g_s, acc=g_acc, msgs=g_msgs), np.random.default_rng(2))


def test_launch_truths_compose_to_the_chain_backward(oracle_mod):
    """depth_bwd followed by sweep_bwd over the stored states equals oracle.mrf_backward's own
    chain from the clipped column on: the launch truths cut the chain where the kernels do."""
    from oracle import mrf_backward as mb
    from test_mrf_backward import make_problem
    o, vg, starts, ends, rvi, rvc, S, planes = make_problem(oracle_mod, seed=1)
    G = np.random.default_rng(5).standard_normal((len(S), rvi.shape[1]))
    args = (vg, rvi, rvc, starts, ends, o.grid_shape)
    _, k = mb.forward(S, *args, iters=2, keep=True, planes=planes)
    Sr = np.zeros(G.shape)
    for r, ray in enumerate(k["rays"]):
        if ray is not None:
            Sr[r, :ray["c"]] = ray["s"]
    accs, msgs = k["accs"], k["msgs"]
    g_s, g_acc, g_m = mt.depth_bwd(Sr, rvi, rvc, accs[2], msgs[2], G)
    prior_bar = g_acc.sum()
    for it in (1, 0):
        d_s, g_acc, g_m = mt.sweep_bwd(Sr, rvi, rvc, accs[it], msgs[it], g_m, g_acc)
        g_s += d_s
        prior_bar += g_acc.sum()
    # the chain's own continuation from dL/dSr to dL/dS: clip + renorm, mapping
    dS = np.zeros(S.shape)
    for r, ray in enumerate(k["rays"]):
        if ray is None:
            continue
        sb, s, y, x, z = g_s[r, :ray["c"]], ray["s"], ray["y"], ray["x"], ray["z"]
        ybar = (sb - (sb * s).sum()) / y.sum()
        xbar = ybar * ((x > mb.LO_S) & (x < mb.HI_S))
        zbar = (xbar - (xbar * x).sum()) / z.sum()
        np.add.at(dS[r], ray["left"], ray["c1"] * zbar)
        np.add.at(dS[r], ray["left"] + 1, ray["c2"] * zbar)
    ref, ref_prior = mb.backward(G, S, *args, iters=2, planes=planes, with_prior=True)
    assert np.abs(dS - ref).max() <= 1e-12 * np.abs(ref).max()
    assert abs(prior_bar - ref_prior) <= 1e-12 * max(1.0, abs(ref_prior))


def measure_fp32(regime):
    """Worst error of the restatement per (mode, output) over FP32_LENGTHS x FP32_DRAWS and the
    GPU tests' launches, with the row length that produced it (-M: the GPU launch at that M)."""
    worst = {}
    launches = [(length, mt.make_launch([length] * mt.FP32_DRAWS, length, regime, seed=1000 + li))
                for li, length in enumerate(mt.FP32_LENGTHS)]
    launches += [(-M, mt.gpu_launch(M, regime)) for M in sorted(mt.GPU_COUNTS)]
    for length, p in launches:
        for mode, name in enumerate(mt.MODES):
            if mode == 0:
                ref = mt.sweep_bwd(p["Sr"], p["rvi"], p["rvc"], p["acc"], p["msgs"], p["g_out"],
                                   p["g_acc_out"])
            else:
                ref = mt.depth_bwd(p["Sr"], p["rvi"], p["rvc"], p["acc"], p["msgs"], p["g_out"])
            got = mt.launch_fp32(mode, p)
            for output, g, t in zip(("gs", "gacc", "gmsgs"), got, ref):
                assert np.isfinite(g).all()
                err = mt.output_error(name, output, regime, g, t, p["rvc"])
                if err >= worst.get((name, output), (-1.0, 0))[0]:
                    worst[name, output] = (err, length)
    return worst


@pytest.mark.parametrize("regime", mt.REGIMES)
def test_fp32_restatement_error(regime):
    """The restatement stays within the recorded E_* of every (mode, output, regime); per ray
    for g_s and g_msgs, per launch for g_acc, and per launch for dL/ds of the depth backward in
    the saturated regime (mrf_bwd_truth.LAUNCH_WIDE says why)."""
    worst = measure_fp32(regime)
    for (mode, output), (err, length) in sorted(worst.items()):
        print("E_%s_%s_%s = %.3e  (row length %d)" % (mode.upper(), output.upper(), regime.upper(),
                                                     err, length))
    for (mode, output), (err, length) in worst.items():
        bound = mt.E(mode, output, regime)
        assert err <= bound, (mode, output, regime, err, length)
        # a recorded constant is a measurement, not a budget: it is the value seen, rounded up
        assert bound <= 1.25 * err + 1e-9, (mode, output, regime, err, bound)
        # and 16 x it, the GPU tolerance, stays below half the chain tolerance
        assert mt.GPU_FACTOR * bound <= 1e-3 or (mode, output, regime) in mt.LAUNCH_WIDE


def test_the_launch_wide_combination_is_small_on_the_launch_scale():
    assert mt.GPU_FACTOR * mt.E_DEPTH_GS_SATURATED <= 1e-3


@pytest.mark.parametrize("regime", mt.REGIMES)
def test_generator_conditions(regime):
    counts = [0, 1, 2, 3, 63, 64, 65, 192, 192]
    p = mt.make_launch(counts, 192, regime, seed=3)
    mt.check_launch(p, counts, 192)             # distinct voxels inside the grid, counts, band
    assert p["Sr"].dtype == np.float32 and p["rvi"].dtype == np.int32 and p["rvc"].dtype == np.int32
    valid = np.arange(192)[None, :] < p["rvc"][:, None]
    assert not p["Sr"][~valid].any() and not p["msgs"][~valid].any()
    lin = np.ravel_multi_index(tuple(p["rvi"][valid].T), p["grid"])
    assert len(np.unique(lin)) < valid.sum()    # rows share voxels
    mu = np.abs(p["acc"].ravel()[lin] - p["msgs"][valid])
    if regime == "prior":
        assert mu.max() < 6 and np.median(p["acc"].ravel()[lin] - p["msgs"][valid]) < -2.5
    if regime == "empty":
        assert mu.max() < mt.BAND[0] and mu.min() > 4
    if regime == "saturated":
        frac = (mu > 12).mean()
        assert 0.05 < frac < 0.15 and mu.max() <= 20.01
    if regime == "mixed":
        assert mu.max() < mt.BAND[0] and (mu > 2).mean() > 0.2
