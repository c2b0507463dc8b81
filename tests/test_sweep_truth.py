"""The truth of tests/sweep_truth.py held on the CPU, before any launch is measured against it:
the fp32 oracle (the reference's arithmetic, restated) lies within the bound at EVERY entry of
every case tests/test_sweep_launches_gpu.py runs; each mutant fails the bound in the regime made
for it; and the flat features of the older sweep tests do not see a wrong softmax maximum -- the
recorded reason why the regimes exist."""
import numpy as np
import pytest

import sweep_truth as T
from mrf_bwd_truth import clip_and_renorm_f32

CASES = []
for _f, _o, _c in T.launch_cases():
    if _c not in CASES:
        CASES.append(_c)


def _wide(D, N, regime, padding=11):
    return T.Case("wide", D, N, 32, padding, regime)


def _column_ratio(b, got):
    S, tol = T.column_truth(b.feats, b.idx, b.o.F)
    return T.worst_ratio(got, S, tol)


def _mapped_ratio(b, got, chained=True):
    """Worst ratio of a mapped [n, M] array over every ray with a voxel, against the truth chained
    from the plane column's."""
    _, _, Sv, tv, _, _ = T.truths(b, chained=chained)
    return max(T.worst_ratio(got[r, :b.rvc[r]], Sv[r], tv[r]) for r in range(len(b.ridx)) if b.rvc[r] >= 1)


# ------------------------------------------------------------------ the reference within the bound
@pytest.mark.parametrize("regime", T.REGIMES)
def test_oracle_lies_within_the_bound_at_every_entry(oracle_mod, regime):
    worst = dict(column=0.0, mapped=0.0, resident=0.0)
    cases = [c for c in CASES if c.regime == regime]
    assert cases
    for case in cases:
        b = T.build(oracle_mod, case)
        S, tolS, Sv, tv, Sr, tr = T.truths(b)
        So = b.o.similarities(b.feats, b.P, b.starts, b.ends)
        assert np.isfinite(So).all(), T.case_id(case)
        w = dict(column=T.worst_ratio(So, S, tolS), mapped=0.0, resident=0.0)
        Svo = b.o.planes_to_voxels(b.vg, b.rvi, b.rvc, b.starts, b.ends, So)
        for r in range(len(b.ridx)):
            cnt = int(b.rvc[r])
            assert np.all(Svo[r, cnt:] == 0)
            if cnt < 1:
                continue
            w["mapped"] = max(w["mapped"], T.worst_ratio(Svo[r, :cnt], Sv[r], tv[r]))
            w["resident"] = max(w["resident"],
                                T.worst_ratio(clip_and_renorm_f32(Svo[r, :cnt]), Sr[r], tr[r]))
        for k in w:
            assert w[k] <= 1.0, (T.case_id(case), k, w[k])
            worst[k] = max(worst[k], w[k])
    print("oracle / bound, %-8s (%2d cases): column %.3f  mapped %.3f  resident %.3f"
          % (regime, len(cases), worst["column"], worst["mapped"], worst["resident"]))


def test_the_cases_hold_what_the_launch_tests_need(oracle_mod):
    """61 rays: odd, no multiple of 4; at most a fifth of them with <= 1 voxels, but some, of both
    kinds; the regimes' spreads as sweep_truth states them."""
    b = T.build(oracle_mod, _wide(64, 5, "flat"))
    n = len(b.ridx)
    short = b.rvc <= 1
    assert n == 61 and 0 < short.sum() <= n // 5
    assert (b.rvc == 0).any() and (b.rvc == 1).any() and np.array_equal(np.where(short)[0], T.SHORT_SLOTS)
    spread = {}
    for regime in ("flat", "peaky", "extreme", "offset", "ramp"):
        b = T.build(oracle_mod, _wide(64, 5, regime))
        x, _, P = T.scores(b.feats, b.idx)
        x = x / P
        spread[regime] = (x.max(1) - x.min(1)).max()
        if regime == "offset":
            assert x.min() > 88.73                      # exp overflows unless the maximum comes off
        if regime == "ramp":
            mx = x.max(1)
            apart = [np.ptp(mx[i:i + 2]) for i in range(0, n - 1, 2)]
            assert np.median(apart) > 40 and max(apart) > 104
    print("score spread within a column:", {k: round(float(v), 2) for k, v in spread.items()})
    assert spread["flat"] < 2 and spread["offset"] < 2
    assert 20 < spread["peaky"] < 80 and spread["ramp"] < 80 and spread["extreme"] > 103.28


# ------------------------------------------------------------------ mutants
def test_the_unmutated_fp32_column_passes_everywhere(oracle_mod):
    """The control of the mutants: their fp32 arithmetic without a mutation is within the bound."""
    for case in (_wide(27, 9, "flat"), _wide(100, 9, "peaky"), _wide(27, 9, "offset"),
                 _wide(27, 9, "ramp"), _wide(100, 9, "extreme")):
        b = T.build(oracle_mod, case)
        assert _column_ratio(b, T.column_plain(b)) <= 1.0, T.case_id(case)
        assert _mapped_ratio(b, T.mapped_plain(b, T.column_truth(b.feats, b.idx, b.o.F)[0])) <= 1.0


@pytest.mark.parametrize("D,N,group", [(9, 9, 4), (16, 3, 4), (27, 9, 2), (32, 5, 2)])
def test_mutant_1_a_neighbouring_rays_maximum(oracle_mod, D, N, group):
    b = T.build(oracle_mod, _wide(D, N, "ramp"))
    assert _column_ratio(b, T.mutant_neighbour_max(b, group)) > 1.0
    b = T.build(oracle_mod, _wide(D, N, "flat"))
    assert _column_ratio(b, T.mutant_neighbour_max(b, group)) <= 1.0       # flat does not see it


@pytest.mark.parametrize("D,N", [(9, 9), (32, 5), (100, 9)])
def test_mutant_2_no_maximum_subtracted(oracle_mod, D, N):
    b = T.build(oracle_mod, _wide(D, N, "offset"))
    assert _column_ratio(b, T.mutant_no_max(b)) > 1.0
    b = T.build(oracle_mod, _wide(D, N, "flat"))
    assert _column_ratio(b, T.mutant_no_max(b)) <= 1.0                     # flat does not see it


@pytest.mark.parametrize("D,N", [(65, 2), (100, 9), (128, 6), (129, 7)])
def test_mutant_3_the_first_chunk_of_planes_only(oracle_mod, D, N):
    """Maximum and sum over the first 64 planes fail in `peaky` at D > 64 -- and, since the SUM is
    short, in `flat` at D > 64 too: there the mutant passes only where it changes nothing
    (D <= 64).  What flat features do hide is the MAXIMUM taken over the first chunk (3b): by shift
    invariance it passes in `flat` and even in `peaky` (spread 26 ... 73 < 88.7, nothing
    overflows); `extreme` sees it where a column's maximum lies past plane 63."""
    b = T.build(oracle_mod, _wide(D, N, "peaky"))
    assert _column_ratio(b, T.mutant_first_chunk(b)) > 1.0
    assert _column_ratio(b, T.mutant_first_chunk_max(b)) <= 1.0
    b = T.build(oracle_mod, _wide(D, N, "flat"))
    assert _column_ratio(b, T.mutant_first_chunk(b)) > 1.0
    assert _column_ratio(b, T.mutant_first_chunk_max(b)) <= 1.0            # flat does not see it
    b = T.build(oracle_mod, _wide(64, 5, "flat"))
    assert _column_ratio(b, T.mutant_first_chunk(b)) <= 1.0
    if D >= 128:            # (the maximum of some column lies past plane 63, > 88.7 above the rest)
        b = T.build(oracle_mod, _wide(D, N, "extreme"))
        assert _column_ratio(b, T.mutant_first_chunk_max(b)) > 1.0


@pytest.mark.parametrize("mutant", [T.mutant_pair_dropped, T.mutant_pair_count, T.mutant_rolled,
                                    T.mutant_padding_counted], ids=lambda m: m.__name__)
@pytest.mark.parametrize("D,N", [(9, 9), (27, 9), (100, 9), (17, 2)])
def test_mutants_4_to_7_fail_in_flat(oracle_mod, mutant, D, N):
    b = T.build(oracle_mod, _wide(D, N, "flat"))
    assert _column_ratio(b, mutant(b)) > 1.0


@pytest.mark.parametrize("mutant", [T.mutant_right_clamped, T.mutant_sum_over_M],
                         ids=lambda m: m.__name__)
@pytest.mark.parametrize("D,N", [(9, 9), (64, 5)])
def test_mutants_8_and_9_fail_in_flat(oracle_mod, mutant, D, N):
    b = T.build(oracle_mod, _wide(D, N, "flat"))
    S = T.column_truth(b.feats, b.idx, b.o.F)[0]
    assert _mapped_ratio(b, T.mapped_plain(b, S)) <= 1.0
    assert _mapped_ratio(b, mutant(b, S)) > 1.0


# ------------------------------------------------------------------ exact columns
@pytest.mark.parametrize("regime", ["constant", "zero"])
def test_exact_columns(oracle_mod, regime):
    for case in (c for c in CASES if c.regime == regime):
        b = T.build(oracle_mod, case)
        S, tol = T.column_truth(b.feats, b.idx, b.o.F)
        assert np.isfinite(S).all() and np.isfinite(tol).all()
        assert np.abs(S - 1.0 / b.o.D).max() <= 1e-15
        So = b.o.similarities(b.feats, b.P, b.starts, b.ends)
        assert np.isfinite(So).all() and np.all(np.abs(So - 1.0 / b.o.D) <= tol)
        if regime == "zero":
            assert np.signbit(b.feats).any() and not b.feats.any()
