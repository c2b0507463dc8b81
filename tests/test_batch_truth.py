"""tests/batch_truth.py, the CPU statement of rn_batch_rays, held to a float64 statement of the
same geometry, to the host routine it replaces (target_points_for_rays) and to the C oracle's
sample_in_bbox -- on every pixel of the seven mock Restrepo views looking at the plane z = 0.3
(N = 5, D = 32, 11 x 11 patches).  No GPU."""
import numpy as np
import pytest

import batch_truth as bt
from conftest import GOLDEN

N, D, PATCH = 5, 32, (11, 11)


@pytest.fixture(scope="module")
def everything():
    scene = bt.plane_scene(GOLDEN)
    cams, nbr = bt.tables(scene, N)
    bbox = np.asarray(scene.bbox, np.float32).ravel()
    view = np.repeat(np.arange(bt.VIEWS), bt.H * bt.W).astype(np.int32)
    ridx = np.tile(np.arange(bt.H * bt.W), bt.VIEWS).astype(np.int32)
    depth = np.concatenate([scene.get_depth_map(v).T.ravel() for v in range(bt.VIEWS)])
    args = (view, ridx, depth, cams, nbr, bbox, bt.H, bt.W, D, PATCH)
    return scene, args, bt.batch_rays_f32(*args), bt.batch_rays_f64(*args)


def test_the_fp32_statement_is_the_fp64_statements_discrete_twin(everything):
    _, args, t32, t64 = everything
    n = len(args[0])
    samples = n * N * D
    tie, face = t64["tie"], t64["face"]
    # the excused samples are few: the float64 statement decides nearly everything
    assert tie.sum() <= 1e-3 * samples, (tie.sum(), samples)
    assert face.sum() <= 1e-3 * n
    differ = (t32["centres"] != t64["centres"]).any(-1)
    print("samples within %g px of a tie: %.4f %%; fp32 centres differing: %.4f %%"
          % (bt.TIE_PX, 100.0 * tie.mean(), 100.0 * differ.mean()))
    assert not (differ & ~tie).any(), int((differ & ~tie).sum())
    # flags: a ray is excused where its target sits on a face or one of its samples on a tie
    excused = face | tie.any((1, 2))
    bad = (t32["flags"] != t64["flags"]) & ~excused
    assert not bad.any(), (int(bad.sum()), t32["flags"][bad][:8], t64["flags"][bad][:8])
    assert np.abs(t32["points"] - t64["points"]).max() < 1e-4
    assert np.abs(t32["target"] - t64["target"]).max() < 1e-4


def test_the_class_mix_the_gpu_tests_rely_on(everything):
    _, args, t32, _ = everything
    flags, view = t32["flags"], args[0]
    assert 0.5 < (flags == 0).mean() < 0.8
    assert 0.1 < ((flags & bt.BORDER) != 0).mean() < 0.4
    assert 0.08 < ((flags & bt.TARGET_OUTSIDE) != 0).mean() < 0.3
    for v in range(bt.VIEWS):
        misses = ((flags[view == v] & bt.MISSES_BOX) != 0).sum()
        assert 300 <= misses <= 1500, (v, misses)
    assert ((flags & bt.NO_DEPTH) != 0).sum() == 0          # the plane is seen everywhere: plant them


def test_planted_depths_set_the_no_depth_bit_only_where_planted(everything):
    _, args, t32, _ = everything
    args = list(args)
    depth = args[2].copy()
    depth[0:16], depth[16:32], depth[32:48], depth[48:64] = 0.0, np.nan, np.inf, 1e6
    args[2] = depth
    got = bt.batch_rays_f32(*args)
    assert np.all((got["flags"][:48] & bt.NO_DEPTH) != 0)
    assert np.all((got["flags"][48:64] & (bt.NO_DEPTH | bt.TARGET_OUTSIDE)) == bt.TARGET_OUTSIDE)
    assert np.array_equal(got["flags"][64:], t32["flags"][64:])
    # a ray without depth: the target is the camera centre
    assert np.array_equal(got["target"][:48, :3], args[3][args[0][:48], 12:15])


def test_targets_are_target_points_for_rays(everything):
    from raynet_amd.train_network.raynet_batch_provider import target_points_for_rays
    scene, args, t32, _ = everything
    view, ridx = args[0], args[1]
    worst = 0.0
    for v in range(bt.VIEWS):
        sel = view == v
        want, valid = target_points_for_rays(scene, v, ridx[sel])
        mine_valid = (t32["flags"][sel] & (bt.NO_DEPTH | bt.TARGET_OUTSIDE)) == 0
        got = t32["target"][sel][:, :3]
        # 4 ulp of the coordinate's magnitude: target_i = step_i + centre_i is a sum of two terms
        # of size ~10 whose result may be small (z = 0.3 from centre_z = 8.4), so the magnitude
        # that sets the rounding error is that of the sum's terms, max(|centre_i|, |target_i|).
        # Measured: the two fp32 routines differ by <= 3 such ulp and each is ~2 ulp(depth) from
        # float64; against ulp(|target_i|) alone the z coordinate is 128 x over, for both.
        centre = np.abs(args[3][v, 12:15])
        tol = 4 * np.spacing(np.maximum(np.abs(want), centre).astype(np.float32))
        both = valid & mine_valid
        assert both.sum() > 0.5 * sel.sum()
        err = np.abs(got[both] - want[both])
        worst = max(worst, float((err / np.maximum(tol[both], 1e-30)).max()))
        assert np.all(err <= tol[both]), (v, float((err / tol[both]).max()))
        # the verdicts agree except where a coordinate sits within those 4 ulp of a face
        bbox = args[5]
        near = (np.abs(got - bbox[:3]) <= 1e-5).any(1) | (np.abs(got - bbox[3:]) <= 1e-5).any(1)
        assert np.all((valid == mine_valid) | near)
    print("targets: worst error %.2f of the 4-ulp tolerance" % worst)


def test_sample_points_twin_against_the_c_oracle(everything, oracle_mod):
    scene, args, t32, _ = everything
    view, ridx, cams, bbox = args[0], args[1], args[3], args[5]
    o = oracle_mod.Oracle(M=32, D=D, N=N, F=4, H=bt.H, W=bt.W, padding=11, bbox=bbox,
                          grid_shape=(8, 8, 8))
    for v in (0, 3, 6):
        sel = view == v
        s, e = o.sample(ridx[sel], cams[v, :12], cams[v, 12:16])
        pts = t32["points"][sel]
        same = lambda a, b: np.array_equal(a.view(np.int32), b.view(np.int32)) or \
            np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
        assert same(pts[:, 0, :3], s)
        # plane D - 1 is s + (D - 1) (e - s) / (D - 1): e up to that expression's rounding
        ok = np.isfinite(e).all(1)
        assert np.abs(pts[ok, -1, :3] - e[ok]).max() < 1e-5
