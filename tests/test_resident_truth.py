"""tests/resident_truth.py held to closed forms, and the conditions every fixture of
tests/test_resident_sweeps_gpu.py meets -- asserted here, on the CPU, from the float64 reference
alone.  No GPU."""
import numpy as np
import pytest

import mrf_bwd_truth as T
import resident_truth as R
import scatter_truth

f32 = np.float32


# ------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("c,a", [(2, -3.0), (7, -1.0), (64, -6.5), (65, -2.0), (300, -6.5)])
def test_constant_occupancy_flat_column(c, a):
    """One occupancy o for every voxel and a flat column s: T_i = (1 - o)^i, w_i = o (1 - o)^i s,
    so C_i = s (1 - q^i), U_i = s (q^(i+1) - q^c): pos_i = s and neg_i = s (1 - q^(c-1)) for
    EVERY i -- all messages are -log(1 - q^(c-1)); and d_i = o q^i / (1 - q^c)."""
    grid = R.GRID
    rvi = np.stack(np.unravel_index(np.arange(c) * 3 % 1170, grid), -1)[None].astype(np.int32)
    assert len(np.unique(np.ravel_multi_index(tuple(rvi[0].T), grid))) == c
    s = f32(1.0 / c)
    Sr = np.full((1, c), s, f32)
    acc = R.uniform(a, grid)
    msgs = np.zeros((1, c), f32)
    o = 1.0 / (1.0 + np.exp(-float(f32(a))))
    q = 1.0 - o
    m, acc_out = T.sweep_fwd(Sr, rvi, np.array([c], np.int32), acc, msgs)
    want = -np.log1p(-q ** (c - 1))
    assert np.allclose(m[0], want, rtol=1e-10, atol=0)
    got = acc_out[tuple(rvi[0].T)]
    assert np.allclose(got, want, rtol=1e-10) and np.count_nonzero(acc_out) == c
    d = T.depth_fwd(Sr, rvi, np.array([c], np.int32), acc, msgs)
    assert np.allclose(d[0], o * q ** np.arange(c) / (1.0 - q ** c), rtol=1e-12, atol=0)
    # the same occupancy from messages: acc - msgs = a
    m2, _ = T.sweep_fwd(Sr, rvi, np.array([c], np.int32), R.uniform(a + 1.5, grid), msgs + f32(1.5))
    assert np.allclose(m2[0], -np.log1p(-(1.0 - 1.0 / (1.0 + np.exp(-(float(f32(a + 1.5)) - 1.5)))) ** (c - 1)),
                       rtol=1e-10)


def test_two_voxel_ray_by_hand():
    grid = R.GRID
    rvi = np.array([[[1, 2, 3], [12, 9, 8]]], np.int32)
    Sr = np.array([[0.25, 0.75]], f32)
    acc = np.zeros(grid, f32)
    acc[1, 2, 3], acc[12, 9, 8] = 1.0, -2.0
    msgs = np.array([[0.5, -0.25]], f32)
    o0, o1 = 1 / (1 + np.exp(-0.5)), 1 / (1 + np.exp(1.75))
    w0, w1 = o0 * 0.25, o1 * (1 - o0) * 0.75
    want = [np.log(0.25 / (w1 / (1 - o0))), np.log((w0 + (1 - o0) * 0.75) / w0)]
    m, acc_out = T.sweep_fwd(Sr, rvi, np.array([2], np.int32), acc, msgs)
    assert np.allclose(m[0], want, rtol=1e-13)
    assert np.isclose(acc_out[1, 2, 3], want[0]) and np.isclose(acc_out[12, 9, 8], want[1])
    d = T.depth_fwd(Sr, rvi, np.array([2], np.int32), acc, msgs)
    assert np.allclose(d[0], [w0 / (w0 + w1), w1 / (w0 + w1)], rtol=1e-13)
    # a count beyond the list's length is the list's length; one voxel or none: nothing
    p = dict(rvc=np.array([9, 1, 0], np.int32), M=2)
    assert R.counts_of(p).tolist() == [2, 1, 0]


def test_rows_for_and_bodies():
    """Chunk count -> body, as RN_DISPATCH_CHUNKS states it."""
    assert R.rows_for(128) == [0, 1, 2, 3, 63, 64, 65, 127, 128, 128]
    assert len(R.rows_for(1024)) == 4 + 3 * 16 - 1 + 1
    assert [R.launch_class(M) for M in R.MS] == [2, 4, 6, 8, 12, 16]
    body = {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6, 7: 8, 8: 8, 9: 12, 10: 12, 11: 12, 12: 12,
            13: 16, 14: 16, 15: 16, 16: 16}
    for nch, nb in body.items():
        for count in (max(2, 64 * nch - 63), 64 * nch):
            assert R.body_of(count, 1024) == nb
    # a launch class caps the body: 5 chunks in a 6-chunk launch, 3 and 4 in a 4-chunk launch
    assert R.body_of(320, 384) == 6 and R.body_of(129, 256) == 3 and R.body_of(256, 256) == 4
    assert R.body_of(128, 128) == 2 and R.body_of(135, 128) == 2       # rvc beyond M clamps
    assert R.body_of(700, 768) == 12 and R.body_of(1, 128) is None and R.body_of(0, 128) is None
    for M in R.MS:
        assert max(R.rows_for(M)) == M and R.rows_for(M)[:4] == [0, 1, 2, 3]
        for k in range(1, M // 64 + 1):
            assert {64 * k - 1, 64 * k} <= set(R.rows_for(M))
            assert (64 * k + 1 in R.rows_for(M)) == (64 * k + 1 <= M)


@pytest.mark.parametrize("grid", [R.GRID, R.GRID_LONG, (4, 4, 4), (5, 1, 9)])
def test_brick_index_is_the_layout_of_the_header(grid):
    """[ceil(gx/4)][ceil(gy/4)][ceil(gz/4)][4][4][4] (include/raynet_hip.h), every axis padded up:
    a bijection from the voxels onto the non-padding cells."""
    nb = R.bricks_of(grid)
    size = R.acc_size(grid)
    assert size == nb[0] * nb[1] * nb[2] * 64
    cells = np.arange(size).reshape(nb + (4, 4, 4)).transpose(0, 3, 1, 4, 2, 5).reshape(
        nb[0] * 4, nb[1] * 4, nb[2] * 4)
    X, Y, Z = np.meshgrid(*[np.arange(g) for g in grid], indexing="ij")
    at = R.brick_index(grid, X, Y, Z)
    assert np.array_equal(at, cells[:grid[0], :grid[1], :grid[2]])
    assert np.array_equal(at, scatter_truth.brick_index(X, Y, Z, grid))     # the library's bit form
    assert len(np.unique(at)) == int(np.prod(grid)) and at.min() >= 0 and at.max() < size
    pad = R.padding_mask(grid)
    assert pad.sum() == size - int(np.prod(grid)) and not pad[at].any()
    a = np.random.default_rng(1).standard_normal(grid).astype(f32)
    v = R.to_bricks(a, fill=-5.0)
    assert np.array_equal(R.from_bricks(v, grid), a) and np.all(v[pad] == -5.0)
    assert v[0] == a[0, 0, 0]
    got, stray = scatter_truth.from_bricked(R.to_bricks(a), grid)
    assert np.array_equal(got, a) and stray == 0


def test_long_grid_reaches_brick_255():
    assert (R.GRID_LONG[0] - 1) // 4 == 255 and all(g % 4 for g in R.GRID_LONG + R.GRID)
    for low in R.LONG_CASES:
        for p in (R.bp_launch(R.M_LONG, "mixed", R.GRID_LONG, low),
                  R.depth_launch(R.M_LONG, "empty", R.GRID_LONG, low)):
            x = p["rvi"][..., 0][np.arange(p["M"])[None, :] < R.counts_of(p)[:, None]]
            assert (x.max() < 8) if low else (x.min() >= 1000 and x.max() == 1020)
            assert p["vox"].dtype == np.int32 and p["vox"].min() >= 0


def test_biased_round_trips():
    rng = np.random.default_rng(3)
    acc = (rng.standard_normal(R.GRID) * 6).astype(f32)
    sums, eff = R.biased(acc, R.PRIOR)
    assert sums.dtype == f32 and eff.dtype == f32
    # acc_eff IS the fp32 sum the kernel forms (the float64 sum of two floats is exact)
    assert np.array_equal(eff, (np.float64(R.PRIOR) + sums.astype(np.float64)).astype(f32))
    assert np.array_equal(sums, (acc.astype(np.float64) - np.float64(R.PRIOR)).astype(f32))
    assert np.abs(eff.astype(np.float64) - acc).max() <= 2.0 ** -23 * (np.abs(acc).max() + abs(R.PRIOR))
    # ... and biasing acc_eff again gives acc_eff again: a fixed point after one step
    assert np.array_equal(R.biased(eff, R.PRIOR)[1], eff)
    assert np.array_equal(R.from_bricks(R.to_bricks(sums), R.GRID), sums)


# ------------------------------------------------------------------ conditions on the fixtures
def _all_launches():
    for M, regime in R.BP_CASES:
        yield "bp", R.bp_launch(M, regime)
    for M, regime in R.DEPTH_CASES:
        yield "depth", R.depth_launch(M, regime)
    for low in R.LONG_CASES:
        yield "bp", R.bp_launch(R.M_LONG, "mixed", R.GRID_LONG, low)
        yield "depth", R.depth_launch(R.M_LONG, "empty", R.GRID_LONG, low)


def test_no_entry_in_the_band():
    """No |mu| in 8.7 .. 9.7 in any form a route evaluates: acc - msgs, acc_eff - msgs, the
    uniform accumulators with and without messages, the accumulator alone (first sweep), the
    prior -- the row whose rvc is M + 7 included (its list is M long)."""
    for _, p in _all_launches():
        M, grid = p["M"], p["grid"]
        assert p["rvc"][-1] == M + 7 and R.counts_of(p)[-1] == M and p["rvi"].shape[1] == M
        zero = np.zeros_like(p["msgs"])
        for acc, msgs in ((p["acc"], p["msgs"]), (p["acc_eff"], p["msgs"]),
                          (R.uniform(p["a0"], grid), p["msgs_uniform"]), (R.uniform(p["a0"], grid), zero),
                          (R.uniform(R.PRIOR, grid), zero), (p["acc_first"], zero)):
            assert R.band_free(p, acc, msgs)
        assert not T._in_band(p["acc_first"]).any()
        assert np.array_equal(R.biased(p["acc"])[1], p["acc_eff"])
        # the uniform route's messages reproduce the launch's own mu (to fp32 rounding)
        inside = np.arange(M)[None, :] < R.counts_of(p)[:, None]
        mu = R._voxel_values(p, p["acc"]).astype(np.float64) - p["msgs"]
        mu_u = np.float64(p["a0"]) - p["msgs_uniform"]
        assert np.abs(mu - mu_u)[inside].max() <= 2.0 ** -22 * (np.abs(mu[inside]).max() + abs(p["a0"]))


def test_every_body_is_taken():
    """Every body NB is run by at least two live rows, in the message launches and in the depth
    launches."""
    for kind in ("bp", "depth"):
        rows = {nb: 0 for nb in R.ALL_BODIES}
        for k, p in _all_launches():
            if k == kind and p["grid"] == R.GRID:
                for c in p["rvc"]:
                    nb = R.body_of(c, p["M"])
                    if nb is not None:
                        rows[nb] += 1
        assert all(v >= 2 for v in rows.values()), (kind, rows)


def _depth_truths():
    centers = np.zeros(R.GRID + (3,), f32)           # (the gaps do not depend on the geometry)
    for M, regime in R.DEPTH_CASES:
        p = R.depth_launch(M, regime)
        for form in ("acc", "acc_eff"):
            yield M, regime, form, p, R.depth_truth(p, p[form], p["msgs"], centers, np.zeros(3, f32))


def test_depth_rows_are_sure_and_reach_both_ends():
    """At least 90 % of the live rows of each depth launch have a float64 top-2 gap above twice
    the distribution tolerance, every distribution sums to 1, and every body has a sure row whose
    arg-max lies in its last live chunk and one whose arg-max lies in chunk 0."""
    for form in ("acc", "acc_eff"):
        first = {nb: 0 for nb in R.ALL_BODIES}
        last = {nb: 0 for nb in R.ALL_BODIES}
        for M, regime, f, p, t in _depth_truths():
            if f != form:
                continue
            counts = R.counts_of(p)
            is_live = counts > 1
            assert np.abs(t["d"][is_live].sum(1) - 1).max() < 1e-12
            assert np.all(t["d"][~is_live] == 0) and np.all(t["d"][~R.live(p)] == 0)
            share = t["sure"][is_live].mean()
            assert share >= 0.9, (M, regime, form, share)
            for r in np.nonzero(is_live & t["sure"])[0]:
                nb = R.body_of(counts[r], M)
                chunk = t["arg"][r] // 64
                first[nb] += chunk == 0         # (a body of NB > 1 is only run by rays of several chunks)
                last[nb] += chunk == R.last_live_chunk(counts[r], M)
        assert all(v >= 1 for v in first.values()) and all(v >= 1 for v in last.values()), (form, first, last)


def test_launches_are_shared_and_read_only():
    p = R.bp_launch(384, "mixed")
    assert p is R.bp_launch(384, "mixed")
    with pytest.raises(ValueError):
        p["msgs"][0, 0] = 1.0
    assert set(R.depth_launch(384, "empty")["kinds"]) == set(R.KINDS)
