"""world_size-2 gloo run of the real RayNetForwardPass driver on CPU tensors.

The HIP kernels cannot run here, so each rank's process replaces the factory the driver takes
its context from (perform_raynet_fp) with a host stand-in built on the oracle
(tests/host_backend.py); what is under test is the
multi-GPU logic of forward_pass.py: contiguous ray sharding, zero-initialised local
accumulators, ONE all-reduce per BP iteration with the prior added once after it
(SURVEY.md 8e), and the merge of the per-rank depth slices."""
import faulthandler
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO

H, W, D, M, GRID, VIEWS = 12, 16, 8, 48, (16, 16, 16), 3


def _run(rank, world, port, out_dir, filtered=False):
    if world > 1:
        # a crash in a spawned rank leaves its Python stack on stderr (captured with the test's output)
        faulthandler.enable()
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from host_backend import OracleBackend
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import get_forward_pass_factory
    from raynet_amd.synthetic import make_synthetic_scene
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank,
                                world_size=world)
    scene, bank = make_synthetic_scene(H=H, W=W, n_views=VIEWS, F=8, padding=5, focal=1.5 * H,
                                       device="cpu")
    gp = GenerationParameters(depth_planes=D, neighbors=VIEWS - 1,
                              grid_shape=np.array(GRID, np.int32),
                              max_number_of_marched_voxels=M, padding=5, gamma_mrf=0.05)
    if filtered:
        # filter_out_rays (forward_pass.py:156-165): only pixels with ground truth are cast
        rng = np.random.default_rng(5)
        masks = [(rng.random((H, W)) > 0.35).astype(np.float32) for _ in range(VIEWS)]
        type(scene).get_depth_map = lambda self, i: masks[i]
    from raynet_amd.forward_pass import map_owner
    # The driver takes its context from perform_raynet_fp's closures (as the reference's takes its
    # kernels from there, forward_pass.py:579-590).  This process replaces THAT with a stand-in
    # whose context is the host back end: the product class has no injection hook.
    import raynet_amd.forward_pass as driver_module

    def perform_raynet_fp_on_the_host(M_, D_, N_, F_, H_, W_, padding, bbox, grid_shape, scheme):
        def not_here(*a, **k):
            raise NotImplementedError("K1 / K2 closures: the resident schedule does not call them")
        not_here.context = OracleBackend(M_, D_, N_, F_, H_, W_, padding, bbox, grid_shape)
        return not_here, not_here
    driver_module.perform_raynet_fp = perform_raynet_fp_on_the_host
    fp = get_forward_pass_factory("raynet")(bank, gp, "sample_in_bbox", (H, W), 50,
                                            filter_out_rays=filtered)
    depths = list(fp.forward_pass(scene, (0, VIEWS, 1)))
    # with a process group image k's map is handed out by ONE rank (map_owner; the reference
    # needs it once: forward_pass.py:739-744); the others yield None for it
    owned = np.array([world == 1 or map_owner(k, VIEWS, world) == rank for k in range(VIEWS)])
    assert [d is not None for d in depths] == owned.tolist()
    if filtered:
        for d, m in zip(depths, masks):
            assert d is None or ((d[m == 0] == 0).all() and (d[m != 0] > 0).all())
    depths = [d if d is not None else np.zeros((H, W), np.float32) for d in depths]
    tag = "f" if filtered else ""
    rows = np.array([len(fp.ray_index[r]) for r in range(VIEWS)])
    np.savez(os.path.join(out_dir, "%sw%d_r%d.npz" % (tag, world, rank)), depth=np.stack(depths),
             owned=owned,
             acc=fp.accumulator.numpy(), rows=rows,
             balance=np.array(fp.shard_balance if fp.shard_balance is not None else []))
    if world > 1:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _merged(ranks):
    """The maps the ranks handed out, put together: every image by exactly one rank, its owner."""
    owned = np.stack([rq["owned"] for rq in ranks])
    assert np.all(owned.sum(0) == 1), owned
    merged = np.zeros_like(ranks[0]["depth"])
    for rq in ranks:
        for k in np.where(rq["owned"])[0]:
            merged[k] = rq["depth"][k]
    return merged


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank_forward_pass_matches_single_rank(tmp_path, world):
    out = str(tmp_path)
    _run(0, 1, 0, out)
    mp.spawn(_run, args=(world, _free_port(), out, False), nprocs=world, join=True)
    one = np.load(os.path.join(out, "w1_r0.npz"))
    ranks = [np.load(os.path.join(out, "w%d_r%d.npz" % (world, q))) for q in range(world)]
    r0 = ranks[0]
    assert one["depth"].shape == (VIEWS, H, W)
    # every rank holds the merged accumulator; every map is handed out once
    for rq in ranks[1:]:
        assert np.array_equal(r0["acc"], rq["acc"])
    depth = _merged(ranks)
    # prior counted once: the N-rank accumulator equals the 1-rank one up to fp32 re-association
    assert np.abs(one["acc"] - r0["acc"]).max() < 1e-4
    assert (np.abs(one["depth"] - depth) > 1e-4).mean() < 0.01
    assert np.isfinite(r0["acc"]).all() and (depth > 0).all()
    # every ray owned by exactly one rank; the shards are cut by traversed voxels, not by rays:
    # every rank's share of the scene's voxel visits is within 25 % of the mean on this tiny
    # scene (192 rays per image, cuts on 8-row boundaries)
    rows = np.stack([rq["rows"] for rq in ranks])
    assert np.all(rows.sum(0) == H * W) and np.all(rows > 0)
    bal = r0["balance"].sum(0).astype(np.float64)          # [world] voxel visits per rank
    assert len(bal) == world and np.all(np.abs(bal / bal.mean() - 1) < 0.25), bal
    for rq in ranks[1:]:
        assert np.array_equal(rq["balance"], r0["balance"])


@pytest.mark.timeout(300)
def test_two_rank_filtered_rays_and_patch_rows(tmp_path):
    """The same with `filter_out_rays`: every rank tile-orders the SAME ragged ray list, owns a
    contiguous slice of it, and the merged maps put the depths back at their pixels."""
    out = str(tmp_path)
    _run(0, 1, 0, out, True)
    mp.spawn(_run, args=(2, _free_port(), out, True), nprocs=2, join=True)
    one = np.load(os.path.join(out, "fw1_r0.npz"))
    r0 = np.load(os.path.join(out, "fw2_r0.npz"))
    r1 = np.load(os.path.join(out, "fw2_r1.npz"))
    assert np.array_equal(r0["acc"], r1["acc"])
    assert np.abs(one["acc"] - r0["acc"]).max() < 1e-4
    assert (np.abs(one["depth"] - _merged([r0, r1])) > 1e-4).mean() < 0.01
