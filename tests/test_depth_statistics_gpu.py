"""Confidence, expected depth and depth std out of the depth sweep (rn_scene_depth_stats,
rn_scene_plan.stats / stats_image, RayNetForwardPass.forward_pass(with_statistics=True)).

Definition (include/raynet_hip.h): for a ray with count > 1 voxels, d_i the depth distribution
(the S_new row) and t_i the distance of voxel i's centre from the camera centre,
confidence = max_i d_i (the reported arg-max's d), mu = sum d_i t_i,
sigma = sqrt(max(0, sum d_i (t_i - mu)^2)); count <= 1: 0, the depth, 0.

Bounds of the float64 comparison (a): the kernel sums fp32 products d (t - K) and d (t - K)^2,
K = t_0, per lane and then over a wave tree -- at most 1024 positive terms, each product a few
roundings: an fp32 emulation of these one-pass pivoted sums over 4000 random rows stayed under
3.1 * 2^-24 * t_max for mu and 6.9 * 2^-24 * L^2 for sigma^2 (L = t_max - t_min of the row).
With a 4x margin and room for t itself (fp32 in the kernel, float64 here: 2 ulp of t):
64 * 2^-24 * t_max and 64 * 2^-24 * L^2.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
F32 = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    from raynet_amd import _lib
    _lib.build()
    return torch


def _moments64(d_row, t):
    d = d_row.astype(np.float64)
    mu = float((d * t).sum())
    return mu, float((d * (t - mu) ** 2).sum())


# ---------------------------------------------------------------------------------------- a
def _kernel_case(torch, oracle_mod, M, counts, seed):
    """Caller-made packed lists along x through a (gx, 4, 4) grid: one row per count and kind of
    column (broad / one sharp peak / a peak in the last chunk), random finite accumulator and
    messages.  -> everything the launches need, and the rows' kinds."""
    from raynet_amd.hip_implementations import get_context
    gx = max(M, 8)
    grid = (gx, 4, 4)
    bbox = np.array([-0.05 * gx, -0.2, -0.2, 0.05 * gx, 0.2, 0.2], F32)
    ctx = get_context(M, 8, 2, 4, 8, 8, 3, bbox, grid)
    vg = oracle_mod.voxel_grid_centers(bbox, grid)
    ctx.set_voxel_grid(torch.from_numpy(vg).cuda())
    rng = np.random.default_rng(seed)
    kinds = ("broad", "sharp", "last")
    rows = [(c, k) for c in counts for k in kinds]
    n = len(rows)
    rvi = np.zeros((n, M, 3), np.int32)
    rvc = np.array([c for c, _ in rows], np.int32)
    Sr = np.zeros((n, M), F32)
    for r, (c, kind) in enumerate(rows):
        x0 = int(rng.integers(0, gx - c + 1))
        rvi[r, :c, 0] = x0 + np.arange(c)
        rvi[r, :, 1], rvi[r, :, 2] = rng.integers(0, 4), rng.integers(0, 4)
        if c == 0:
            continue
        s = rng.random(c) + 0.05
        if kind == "sharp":
            s[int(rng.integers(0, c))] += 200.0 * c
        elif kind == "last":
            s[c - 1 - int(rng.integers(0, min(c, 20)))] += 200.0 * c
        Sr[r, :c] = (s / s.sum()).astype(F32)
    packed = ((rvi[..., 0] << 20) | (rvi[..., 1] << 10) | rvi[..., 2]).astype(np.int32)
    # low occupancies: the transmittance still reaches the last chunk of a 650-voxel ray
    acc_grid = rng.uniform(-7.0, -5.0, size=grid).astype(F32)
    msgs = rng.uniform(-1.0, 1.0, size=(n, M)).astype(F32)
    cc = np.array([-0.05 * gx - 2.0, 0.03, -0.02], F32)
    dev = "cuda"
    t = np.linalg.norm(vg[rvi[..., 0], rvi[..., 1], rvi[..., 2]].astype(np.float64) -
                       cc.astype(np.float64), axis=-1)                       # [n, M]
    args = dict(Sr=torch.from_numpy(Sr).to(dev), vox=torch.from_numpy(packed).to(dev),
                rvc=torch.from_numpy(rvc).to(dev), acc=ctx.acc_from_grid(acc_grid),
                msgs=torch.from_numpy(msgs).to(dev), cc=torch.from_numpy(cc).to(dev))
    return ctx, args, rows, rvc, t


@pytest.mark.parametrize("M,counts", [(200, (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)),
                                      (650, (1, 2, 400, 641, 650))])
def test_kernel_against_float64(torch, oracle_mod, M, counts):
    ctx, a, rows, rvc, t = _kernel_case(torch, oracle_mod, M, counts, seed=11 + M)
    n = len(rows)
    S_new = torch.zeros((n, M), device="cuda")
    depth = torch.full((n,), -1.0, device="cuda")
    stats = torch.full((3, n + 5), -7.0, device="cuda")           # (a stride that is not n)
    ctx.scene_depth_stats(a["Sr"], a["vox"], a["rvc"], a["acc"], a["msgs"], a["cc"], S_new, depth,
                          stats)
    S_plain = torch.zeros((n, M), device="cuda")
    depth_plain = torch.full((n,), -1.0, device="cuda")
    ctx.scene_depth(a["Sr"], a["vox"], a["rvc"], a["acc"], a["msgs"], a["cc"], S_plain, depth_plain)
    S, d, st = S_new.cpu().numpy(), depth.cpu().numpy(), stats.cpu().numpy()
    # the depth and the distribution of this launch are rn_scene_depth's, bit for bit
    assert np.array_equal(S, S_plain.cpu().numpy())
    assert np.array_equal(d, depth_plain.cpu().numpy())
    assert np.all(st[:, n:] == -7.0)                              # nothing beyond the n rays
    assert np.isfinite(S).all() and np.isfinite(st).all()
    conf, mean, sd = st[0, :n], st[1, :n], st[2, :n]
    worst_mu = worst_var = 0.0
    for r, (c, kind) in enumerate(rows):
        if c <= 1:                                                # such rays send nothing: section 1
            assert conf[r] == 0.0 and sd[r] == 0.0 and mean[r] == d[r], (c, kind)
            continue
        assert conf[r] == S[r].max(), (c, kind)                   # bit for bit
        tt = t[r, :c]
        mu64, var64 = _moments64(S[r, :c], tt)
        L = tt.max() - tt.min()
        e_mu = abs(float(mean[r]) - mu64) / (EPS * tt.max())
        e_var = abs(float(sd[r]) ** 2 - var64) / (EPS * L * L)
        print("M=%d count=%d %s: |mu - mu64| = %.2f, |var - var64| = %.2f (units of 2^-24 t_max, "
              "2^-24 L^2), conf %.3g" % (M, c, kind, e_mu, e_var, conf[r]))
        worst_mu, worst_var = max(worst_mu, e_mu), max(worst_var, e_var)
        assert e_mu <= 64.0, (c, kind, e_mu)
        assert e_var <= 64.0, (c, kind, e_var)
    print("worst: mu %.2f, var %.2f" % (worst_mu, worst_var))


def test_stats_are_required(torch, oracle_mod):
    """stats == NULL is an error of rn_scene_depth_stats, not a plain depth sweep."""
    import ctypes
    from raynet_amd import _lib
    ctx, a, rows, rvc, t = _kernel_case(torch, oracle_mod, 200, (2, 64), seed=5)
    n = len(rows)
    depth = torch.full((n,), -1.0, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = ctx.lib.rn_scene_depth_stats(ctx._h, n, p(a["Sr"]), p(a["vox"]), p(a["rvc"]), p(a["acc"]),
                                      p(a["msgs"]), p(a["cc"]), 0, None, p(depth), None, n, None)
    torch.cuda.synchronize()
    assert rc == -1 and b"stats" in ctx.lib.rn_last_error(ctx._h)
    assert np.all(depth.cpu().numpy() == -1.0)


# ---------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("case", ["wide", "aniso"])
def test_against_the_oracle(torch, oracle_mod, case):
    """The cases and setup of test_resident_scene_path_equals_fused: confidence within 1e-5 of
    the oracle's S_new.max (the tolerance S_new itself is held to there), the mean within what a
    1e-5 error per entry can move it by: count * 1e-5 * L."""
    from test_hip_parity_gpu import CU, hip_ctx, make_case
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
    acc_o = o.prior(0.05)
    msgs_o = np.zeros((n, o.M), F32)
    for it in range(3):
        out = o.prior(0.05)
        o.fused_bp(c["ray_idxs"], feats, c["P"], c["P_inv"], c["center"], vg, acc_o, msgs_o, out)
        acc_o = out
    depth = torch.zeros((n,), device=dev)
    stats = torch.zeros((3, n), device=dev)
    ctx.scene_depth_stats(Sr, vox, rvc, ctx.acc_from_grid(acc_o), torch.from_numpy(msgs_o).to(dev),
                          cc, None, depth, stats)
    rvi, cnt, S_new_o, depth_o = o.fused_depth(c["ray_idxs"], feats, c["P"], c["P_inv"],
                                               c["center"], vg, acc_o, msgs_o)
    st, d = stats.cpu().numpy(), depth.cpu().numpy()
    assert np.abs(st[0] - S_new_o.max(axis=1)).max() <= 1e-5
    t = np.linalg.norm(vg[rvi[..., 0], rvi[..., 1], rvi[..., 2]].astype(np.float64) -
                       np.asarray(c["center"], np.float64).ravel()[:3], axis=-1)
    checked = 0
    for r in range(n):
        k = int(min(cnt[r], o.M))
        if k <= 1:
            assert st[0, r] == 0.0 and st[2, r] == 0.0 and st[1, r] == d[r]
            continue
        mu_o, _ = _moments64(S_new_o[r, :k], t[r, :k])
        L = t[r, :k].max() - t[r, :k].min()
        assert abs(float(st[1, r]) - mu_o) <= k * 1e-5 * L, (r, k, st[1, r], mu_o)
        assert t[r, :k].min() * (1 - 1e-6) <= st[1, r] <= t[r, :k].max() * (1 + 1e-6)
        assert 0.0 <= st[2, r] <= L
        checked += 1
    assert checked > n // 2


# ---------------------------------------------------------------------------------------- c, d
def _gp(D, M, grid, neighbors=4, padding=11):
    from raynet_amd.common.generation_parameters import GenerationParameters
    return GenerationParameters(depth_planes=D, neighbors=neighbors,
                                grid_shape=np.array(grid, np.int32),
                                max_number_of_marched_voxels=M, padding=padding, gamma_mrf=0.05)


H, W, V = 48, 64, 5


def _small_scene():
    from raynet_amd.synthetic import make_synthetic_scene
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=5, focal=1.5 * H)
    return scene, bank, _gp(32, 192, (64, 64, 64))


def _pass(fp, scene, with_statistics=True):
    """-> [V, 4, H, W] (depth, confidence, expected depth, std) COPIES of one pass, or [V, H, W]"""
    if not with_statistics:
        return np.stack([m.copy() for m in fp.forward_pass(scene, (0, V, 1))])
    return np.stack([np.stack([d.copy()] + [m.copy() for m in s])
                     for d, s in fp.forward_pass(scene, (0, V, 1), with_statistics=True)])


@pytest.fixture(scope="module")
def small(torch):
    """The small shape of test_plan_path_equals_the_launch_by_launch_path, fixed-point sums: the
    plan path's four maps of every image, computed once and left alone."""
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.hip_implementations.options import PathOptions
    scene, bank, gp = _small_scene()
    cls = get_forward_pass_factory("raynet")
    fp = cls(bank, gp, "sample_in_bbox", (H, W), 0, options=PathOptions(deterministic=True))
    maps = _pass(fp, scene)
    assert fp._plan["fast"] is not None and fp._plan["direct"] and fp._plan["with_stats"]
    maps.setflags(write=False)
    return dict(scene=scene, bank=bank, gp=gp, cls=cls, fp=fp, maps=maps)


def test_pixel_order_and_padding(torch, small):
    """rn_scene_run with a pixel-order destination: every statistics plane, indexed by ray_idxs,
    is the row-order plane; entries no ray maps to keep their sentinel; padding rows are written
    in row order (as depth[] is) and nowhere in pixel order."""
    from raynet_amd import _lib
    fp, ctx = small["fp"], small["fp"]._ctx
    pl0 = fp._plan
    nv, M, dev = 3, fp._rows_M(), "cuda"
    g = torch.Generator().manual_seed(3)
    n = H * W - 500                                   # some pixels without a ray; n % 256 != 0
    ridx = torch.randperm(H * W, generator=g)[:n].to(torch.int32).to(dev)
    npad = (n + 255) // 256 * 256
    rows, G = nv * npad, ctx.acc_size()
    buf = dict(vox=torch.zeros((rows, M), dtype=torch.int32, device=dev),
               rvc=torch.zeros((rows,), dtype=torch.int32, device=dev),
               Sr=torch.zeros((rows, M), device=dev), msgs=torch.zeros((rows, M), device=dev),
               acc0=torch.zeros((G,), device=dev), acc1=torch.zeros((G,), device=dev))

    def plan(depth, **kw):
        return ctx.scene_plan(nv, npad, ridx, pl0["table"][:nv], pl0["cam_dev"][:nv], buf["vox"],
                              buf["rvc"], buf["Sr"], buf["msgs"], buf["acc0"], buf["acc1"], depth,
                              pl0["prior"], False, **kw)

    depth_rows = torch.full((rows,), -5.0, device=dev)
    stats_rows = torch.full((3, rows), -7.0, device=dev)
    by_rows = plan(depth_rows, stats=stats_rows)
    ctx.scene_run(by_rows, _lib.RN_RUN_PREPARE | _lib.RN_RUN_SWEEP, 0)
    ctx.scene_run(by_rows, _lib.RN_RUN_SWEEP, 1)
    ctx.scene_run(by_rows, _lib.RN_RUN_DEPTH_RANGE, 2, 0 | (2 << 16))
    ctx.scene_run(by_rows, _lib.RN_RUN_DEPTH, 2, 2)
    # the same launches without statistics: the depths of today, in the entries of today (the
    # one-image form sweeps the image's n rays, not its padding rows)
    depth_plain = torch.full((rows,), -5.0, device=dev)
    plain = plan(depth_plain)
    ctx.scene_run(plain, _lib.RN_RUN_DEPTH_RANGE, 2, 0 | (2 << 16))
    ctx.scene_run(plain, _lib.RN_RUN_DEPTH, 2, 2)
    assert torch.equal(depth_plain, depth_rows)
    # ... and the sweep of all images at once gives every ray the same depth
    depth_all = torch.full((rows,), -5.0, device=dev)
    ctx.scene_run(plan(depth_all), _lib.RN_RUN_DEPTH, 2, -1)
    assert torch.equal(depth_all.view(nv, npad)[:, :n], depth_rows.view(nv, npad)[:, :n])
    assert torch.equal(depth_all[:2 * npad], depth_rows[:2 * npad])
    maps = torch.full((nv, H * W), -5.0, device=dev)
    stats_img = torch.full((3, nv, H * W), -7.0, device=dev)
    by_pixels = plan(torch.full((rows,), -5.0, device=dev), depth_image=maps, stats_image=stats_img)
    ctx.scene_run(by_pixels, _lib.RN_RUN_DEPTH_RANGE, 2, 0 | (2 << 16))
    ctx.scene_run(by_pixels, _lib.RN_RUN_DEPTH, 2, 2)
    torch.cuda.synchronize()
    sr = stats_rows.view(3, nv, npad)
    dr = depth_rows.view(nv, npad)
    idx = ridx.long()
    assert torch.equal(maps[:, idx], dr[:, :n])
    for p in range(3):
        assert torch.equal(stats_img[p][:, idx], sr[p, :, :n]), p
    hit = torch.zeros((H * W,), dtype=torch.bool, device=dev)
    hit[idx] = True
    assert int((~hit).sum()) == 500
    assert bool((stats_img[:, :, ~hit] == -7.0).all()) and bool((maps[:, ~hit] == -5.0).all())
    # padding rows (count 0) of the range launch: written in row order like their depth --
    # confidence 0, mean = depth; those of the one-image launch are not swept, like their depth
    assert bool((dr[:2, n:] != -5.0).all())
    assert bool((sr[0, :2, n:] == 0).all()) and bool((sr[2, :2, n:] == 0).all())
    assert torch.equal(sr[1, :2, n:], dr[:2, n:])
    assert bool((dr[2, n:] == -5.0).all()) and bool((sr[:, 2, n:] == -7.0).all())
    assert float(sr[0, :, :n].max()) > 0.0


def test_drivers_agree(torch, small):
    """Plan path / launch by launch, leased / copied maps, with / without statistics, a second
    pass over the cached plan: the same bits; a leased statistics array survives the next pass;
    the values are what they claim to be."""
    from raynet_amd.hip_implementations.options import PathOptions
    scene, bank, gp, cls, ref = (small[k] for k in ("scene", "bank", "gp", "cls", "maps"))
    fp = small["fp"]
    # a second pass over the cached plan, the first pass's arrays still held (leases)
    held = list(fp.forward_pass(scene, (0, V, 1), with_statistics=True))
    plan = fp._plan
    again = _pass(fp, scene)
    assert fp._plan is plan
    assert np.array_equal(again, ref)
    for k, (d, s) in enumerate(held):                 # ... which the later pass did not overwrite
        assert np.array_equal(d, ref[k, 0])
        for p, m in enumerate(s):
            assert m.shape == (H, W) and m.dtype == np.float32
            assert np.array_equal(m, ref[k, 1 + p]), (k, p)
    del held
    # a plan built without statistics does not serve a pass with them (and the depth maps are
    # the depth maps of a pass without)
    plain = _pass(fp, scene, with_statistics=False)
    assert fp._plan is not plan and not fp._plan["with_stats"]
    assert np.array_equal(plain, ref[:, 0])
    assert np.array_equal(_pass(fp, scene), ref) and fp._plan["with_stats"]
    for opts in (dict(plan_path=False), dict(maps="copy")):
        other = cls(bank, gp, "sample_in_bbox", (H, W), 0,
                    options=PathOptions(deterministic=True, **opts))
        got = _pass(other, scene)
        assert (other._plan["fast"] is None) == (opts.get("plan_path") is False)
        assert np.array_equal(got, ref), opts
        if "plan_path" in opts:
            assert np.array_equal(_pass(other, scene, with_statistics=False), ref[:, 0])
    # what the numbers are
    conf, mean, sd = ref[:, 1], ref[:, 2], ref[:, 3]
    assert conf.min() >= 0.0 and conf.max() <= 1.0 and conf.max() > 0.0
    assert sd.min() >= 0.0 and np.isfinite(ref).all()
    # the mean lies between the nearest and the farthest voxel centre of the ray: a sample of
    # rays, from the traversal the context left in the plan's buffers
    pl = fp._plan
    vg = fp._vg.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(0)
    for k in (0, 3):
        st = pl["per_image"][k]
        ridx = st["ridx"].cpu().numpy()
        cnt = st["rvc"].cpu().numpy()
        cc = st["center"].cpu().numpy().astype(np.float64)[:3]
        for row in rng.choice(len(ridx), 200, replace=False):
            c = int(min(cnt[row], pl["vox"].shape[1]))
            x, y = int(ridx[row]) // H, int(ridx[row]) % H             # ray index = x * H + y
            if c <= 1:
                assert conf[k, y, x] == 0 and sd[k, y, x] == 0 and mean[k, y, x] == ref[k, 0, y, x]
                continue
            pk = pl["vox"][st["row0"] + row, :c].cpu().numpy()
            t = np.linalg.norm(vg[pk >> 20, (pk >> 10) & 1023, pk & 1023] - cc, axis=-1)
            assert t.min() * (1 - 1e-6) <= mean[k, y, x] <= t.max() * (1 + 1e-6), (k, row)
            assert sd[k, y, x] <= t.max() - t.min()
            assert np.abs(t - ref[k, 0, y, x]).min() <= 1e-5 * t.max()   # the depth is one of them


def test_captured_replay_equals_eager(torch, small):
    """The step with statistics recorded into one HIP graph and replayed: the eager bits."""
    from raynet_amd.hip_implementations.options import PathOptions
    scene, bank, gp, cls, ref = (small[k] for k in ("scene", "bank", "gp", "cls", "maps"))
    fp = cls(bank, gp, "sample_in_bbox", (H, W), 0,
             options=PathOptions(deterministic=True, capture="on"))
    seen = []
    # (the adaptive scatter settles within ~40 scatter launches on this scene, see
    # test_captured_step_replays_the_eager_pass)
    for i in range(40):
        got = _pass(fp, scene)
        seen.append(fp.captured)
        assert np.array_equal(got, ref), i
        if sum(seen) >= 2:
            break
    assert seen[-1] and seen[-2] and not seen[0]


# ---------------------------------------------------------------------------------------- e
def _rank_main(rank, world, port, out_dir):
    import sys
    import torch
    import torch.distributed as dist
    from conftest import REPO
    sys.path.insert(0, REPO)
    from raynet_amd.forward_pass import get_forward_pass_factory, map_owner
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank,
                            world_size=world)
    scene, bank, gp = _small_scene()
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 0)
    out = list(fp.forward_pass(scene, (0, V, 1), with_statistics=True))
    assert fp._plan["fixed"] and fp._plan["fast"] is not None
    owned = [k for k in range(V) if map_owner(k, V, world) == rank]
    saved = {"owned": np.array(owned, np.int64)}
    for k, (d, s) in enumerate(out):
        if k in owned:
            saved["maps_%d" % k] = np.stack([d] + list(s))
        else:
            assert d is None and s is None
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), **saved)
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu(torch, small, tmp_path):
    """Two processes (gloo) share the GPU, each with its shard of every image's rays: the
    statistics rows travel as the depth rows do and the owner's four maps are the one-rank
    fixed-point maps, bit for bit."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    seen = []
    for q in range(2):
        z = np.load(os.path.join(str(tmp_path), "r%d.npz" % q))
        for k in z["owned"]:
            assert np.array_equal(z["maps_%d" % int(k)], small["maps"][int(k)]), (q, int(k))
            seen.append(int(k))
    assert sorted(seen) == list(range(V))


# ---------------------------------------------------------------------------------------- f
class _MaskedScene(object):
    """A scene's cameras with ground-truth maps of our own (what _selected_pixels looks at)."""

    def __init__(self, scene, truth):
        self._scene, self._truth = scene, truth

    def get_image(self, i):
        return self._scene.get_image(i)

    def get_depth_map(self, i):
        return self._truth[i]


def test_point_cloud_confidence_threshold(torch, small, tmp_path):
    from raynet_amd import pointcloud as pc
    ref = small["maps"]
    frames, b = [0, 1, 2], 6
    rng = np.random.default_rng(4)
    truth = [(rng.random((H, W)) > 0.1).astype(F32) for _ in frames]      # some pixels unobserved
    scene = _MaskedScene(small["scene"], truth)
    depths = [ref[k, 0].copy() for k in frames]
    confs = [ref[k, 1].copy() for k in frames]
    today = pc.PointcloudFromDepthMaps(scene, frames, depths, borders=b).points
    same = pc.PointcloudFromDepthMaps(scene, frames, depths, borders=b, confidences=confs,
                                      min_confidence=0.0).points
    assert np.array_equal(today, same)
    via = pc.get_pointcloud(scene, frames, depths, False, borders=b, confidences=confs,
                            min_confidence=0.0).points
    assert np.array_equal(today, via)
    thr = float(np.median(np.stack(confs)[:, b:H - b, b:W - b]))
    kept = pc.PointcloudFromDepthMaps(scene, frames, depths, borders=b, confidences=confs,
                                      min_confidence=thr).points
    # the reference's order: frame by frame, the cropped map's boolean selection (row-major)
    keep = np.concatenate([((truth[i][b:H - b, b:W - b] != 0))[truth[i][b:H - b, b:W - b] != 0]
                           & (confs[i][b:H - b, b:W - b] >= thr)[truth[i][b:H - b, b:W - b] != 0]
                           for i in range(len(frames))])
    assert 0 < keep.sum() < keep.size
    assert np.array_equal(kept, today[:, keep])
    files = []
    for i, c in zip(frames, confs):                                       # file names, as depthmaps
        files.append(str(tmp_path / ("confidence_%03d.npy" % i)))
        np.save(files[-1], c)
    from_files = pc.PointcloudFromDepthMaps(scene, frames, depths, borders=b, confidences=files,
                                            min_confidence=thr).points
    assert np.array_equal(from_files, kept)
    with pytest.raises(ValueError):
        pc.PointcloudFromDepthMaps(scene, frames, depths, borders=b, min_confidence=0.5)
