"""sample_in_range and sample_in_disparity on the GPU, through the C ABI's scheme entries
(include/raynet_hip.h, "sampling schemes") and the drivers on top of them,
against tests/sampling_truth.py and the reference's own points
(tests/golden/ref_sampling_schemes_np.npz).

Images are 24 x 32 on the synthetic ring cameras (box [-1, 1]^3, range (2, 4): corner rays miss
the box) and the mock Restrepo cameras (their scene's box, range (3, 7)).  D in {5, 16, 33, 64,
70}: below one chunk of 64 planes, the range the bbox sweep packs, an odd tail, exactly one
chunk, a second chunk.  F in {32, 12}: the cooperative and the generic sweep.  N in {2, 5}.
Ray counts {0, 1, 63, 64, 65, 200}."""
import ctypes
import functools

import numpy as np
import pytest

import batch_truth as bt
import sampling_truth as st
from conftest import GOLDEN, load_cases
from test_sampling_reference import REL_TOL, _scale

pytestmark = pytest.mark.gpu

REF = load_cases("ref_sampling_schemes_np.npz")
DS = (5, 16, 33, 64, 70)
RAY_COUNTS = (0, 1, 63, 64, 65, 200)
PAD = 3
# A distance "in [r0, r1]" in fp32: the coordinates of a sample are below 16 in both scenes (ulp
# 2^-20), each carries at most 6 roundings (d^, s, e, plane_point), the distance three of them and
# its own square root: 6 * sqrt(3) * 2^-20 = 1e-5.
FP32_SLACK = 1e-5
KINDS = ("ring", "restrepo")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    from raynet_amd import _lib
    _lib.build()
    return torch


@functools.lru_cache(maxsize=None)
def _scene(kind):
    return st.scene_of(kind, GOLDEN)


def _ctx(scene, D, N, F, H=st.H, W=st.W):
    from raynet_amd.hip_implementations import get_context
    return get_context(8, D, N, F, H, W, PAD, np.asarray(scene.bbox, np.float32).ravel(), (4, 4, 4))


def _far_view(cam):
    far = cam["far"]
    return far[16:].reshape(3, 4), far[:12].reshape(4, 3), far[12:16]


def _sampling(ctx, scheme, kind, cam):
    return ctx.sampling(scheme, st.RANGES[kind], _far_view(cam))


def _truth_points(scheme, kind, scene, cam, ridx, D):
    bbox = np.asarray(scene.bbox, np.float32).ravel()
    if scheme == "sample_in_range":
        return st.sample_in_range(ridx, st.H, cam["P_inv"], cam["center"], st.RANGES[kind], D)
    return st.sample_in_disparity(ridx, st.H, cam["P_inv"], cam["center"], bbox, cam["far"], D)["points"]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _k8(torch, ctx, sm, ridx, cam, D):
    pts = torch.full((len(ridx), D, 4), -7.0, device="cuda")
    ctx.sample_points_scheme(ctx.dev(ridx), ctx.dev(cam["P_inv"]), ctx.dev(cam["center"]), sm, pts)
    return pts.cpu().numpy()


def _features(N, F, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, st.H + PAD + 1, st.W + PAD + 1, F), dtype=np.float32) * np.float32(0.25)


# ------------------------------------------------------------------ K8
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("kind", KINDS)
def test_k8_points_against_the_truth(torch, kind, D):
    """range: within the bbox test's bound of the NumPy statement; disparity: its bits (fp64 add,
    multiply, divide and the conversions are correctly rounded on the device, -ffp-contract=off)."""
    scene = _scene(kind)
    cam = st.camera_arrays(scene, 0, 5)
    ctx = _ctx(scene, D, 5, 32)
    scale = float(np.abs(np.concatenate([np.asarray(scene.bbox).ravel(), cam["center"][:3]])).max())
    missed_any = False
    for n in RAY_COUNTS:
        ridx = st.rays_with_misses(scene, 0, n, seed=n)
        pr = _k8(torch, ctx, _sampling(ctx, "sample_in_range", kind, cam), ridx, cam, D)
        tr = _truth_points("sample_in_range", kind, scene, cam, ridx, D)
        if n:
            err = np.abs(pr - tr).max()
            print("%s D=%d n=%d range: max |gpu - truth| = %.3g (bound %.3g), same bits: %s"
                  % (kind, D, n, err, REL_TOL * scale, _same_bits(pr, tr)))
            assert err <= REL_TOL * scale
        assert np.all(pr[..., 3] == 1.0)
        pd = _k8(torch, ctx, _sampling(ctx, "sample_in_disparity", kind, cam), ridx, cam, D)
        td = _truth_points("sample_in_disparity", kind, scene, cam, ridx, D)
        if n:
            ok = np.isfinite(td).all(axis=(1, 2))
            print("%s D=%d n=%d disparity: %d missed, max |gpu - truth| = %.3g"
                  % (kind, D, n, int((td[:, 0, 3] == 0).sum()), np.abs(pd[ok] - td[ok]).max()))
        assert _same_bits(pd, td)
        missed = pd[:, 0, 3] == 0
        missed_any |= bool(missed.any())
        assert np.all(np.isfinite(pd[missed])) and np.all(pd[missed][..., :3] == cam["center"][:3])
    assert missed_any                              # rays that miss the box are among them


@pytest.mark.parametrize("case", sorted(REF))
def test_k8_points_against_the_reference(torch, case):
    c = REF[case]
    H, W, D = (int(v) for v in c["HWD"])
    from raynet_amd.hip_implementations import get_context
    ctx = get_context(8, D, 2, 4, H, W, 1, c["bbox"], (4, 4, 4))
    P_inv, centre = c["P_pinv"].astype(np.float32), np.append(c["center"][:3], 1).astype(np.float32)
    far = (c["far_P"].astype(np.float32), c["far_P_pinv"].astype(np.float32), c["far_center"][:3])
    ridx = c["ray_idxs"]
    tol = REL_TOL * _scale(c)

    def run(scheme):
        pts = torch.zeros((len(ridx), D, 4), device="cuda")
        ctx.sample_points_scheme(ctx.dev(ridx), ctx.dev(P_inv), ctx.dev(centre),
                                 ctx.sampling(scheme, c["range"], far), pts)
        return pts.cpu().numpy()
    pr = run("sample_in_range")
    err_r = np.abs(pr[..., :3] - c["points_range"]).max()
    pd = run("sample_in_disparity")
    hit = c["disparity_hit"].astype(bool)
    assert np.array_equal(pd[:, 0, 3] == 0, ~hit)          # the reference's None
    far_row = np.concatenate([far[1].ravel(), far[2], [1], far[0].ravel()]).astype(np.float32)
    par = (st.sample_in_disparity(ridx, H, P_inv, centre, c["bbox"], far_row, D)["parallel"] < 1e-6).any(1)
    keep = hit & ~par
    err_d = np.abs(pd[keep][..., :3] - c["points_disparity"][keep]).max()
    print("%s: range %.3g, disparity %.3g (bound %.3g), %d nearly parallel" % (case, err_r, err_d, tol, par.sum()))
    assert (par & hit).sum() <= 0.02 * len(hit)
    assert err_r <= tol and err_d <= tol


# ------------------------------------------------------------------ K9
def _k9(torch, ctx, sm, ridx, feats, cam, D):
    S = torch.full((len(ridx), D), -7.0, device="cuda")
    ctx.mvcnn_similarities_scheme(ctx.dev(ridx), ctx.dev(feats), ctx.dev(cam["P"]), ctx.dev(cam["P_inv"]),
                                  ctx.dev(cam["center"]), sm, S)
    return S.cpu().numpy()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("F", [32, 12])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_k9_range_is_the_sweep_on_the_range_segment(torch, kind, N, F, D):
    """The same plane_point, the same sweep: rn_compute_similarities' bits on (s, e)."""
    scene = _scene(kind)
    cam = st.camera_arrays(scene, 0, N)
    ctx = _ctx(scene, D, N, F)
    feats = _features(N, F)
    sm = _sampling(ctx, "sample_in_range", kind, cam)
    for n in RAY_COUNTS:
        ridx = st.rays_with_misses(scene, 0, n, seed=D + n)
        s, e = st.range_segment_f32(ridx, st.H, cam["P_inv"], cam["center"], st.RANGES[kind])
        # (s, e) are the device's: K8's points are plane_point on them, bit for bit
        assert _same_bits(_k8(torch, ctx, sm, ridx, cam, D)[..., :3], st.plane_points_f32(s, e, D))
        S = _k9(torch, ctx, sm, ridx, feats, cam, D)
        S_seg = torch.zeros((n, D), device="cuda")
        ctx.compute_similarities(ctx.dev(feats), ctx.dev(cam["P"]), ctx.dev(s), ctx.dev(e), S_seg)
        assert _same_bits(S, S_seg.cpu().numpy())
        assert n == 0 or np.abs(S.sum(1) - 1).max() < 1e-5


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("F", [32, 12])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_k9_disparity_against_the_numpy_sweep(torch, kind, N, F, D):
    """Columns against tests/sampling_truth.py's plane sweep on the truth's points; the bound is
    tests/test_hip_parity_gpu.py's for the sweep against the oracle (2e-6 generic, 1e-5 for the
    cooperative F = 32 sweep, which re-associates the 32-term sums)."""
    scene = _scene(kind)
    cam = st.camera_arrays(scene, 0, N)
    ctx = _ctx(scene, D, N, F)
    feats = _features(N, F)
    sm = _sampling(ctx, "sample_in_disparity", kind, cam)
    tol = 1e-5 if F == 32 else 2e-6
    for n in RAY_COUNTS:
        ridx = st.rays_with_misses(scene, 0, n, seed=D + n)
        S = _k9(torch, ctx, sm, ridx, feats, cam, D)
        assert S.shape == (n, D)
        if n == 0:
            continue
        pts = _truth_points("sample_in_disparity", kind, scene, cam, ridx, D)
        St = st.similarities(pts, feats, cam["P"], st.H, st.W, PAD)
        err = np.abs(S - St).max()
        print("%s N=%d F=%d D=%d n=%d: max |gpu - numpy sweep| = %.3g (bound %.3g)"
              % (kind, N, F, D, n, err, tol))
        assert np.all(np.isfinite(S)) and np.abs(S.sum(1) - 1).max() < 1e-5
        assert err <= tol


# ------------------------------------------------------------------ K10
def _k10(torch, ctx, sm, ridx, feats, cam, D):
    n = len(ridx)
    S = torch.full((n, D), -7.0, device="cuda")
    pts = torch.full((n, D, 4), -7.0, device="cuda")
    depth = torch.full((n,), -7.0, device="cuda")
    ctx.mvcnn_depth_scheme(ctx.dev(ridx), ctx.dev(feats), ctx.dev(cam["P"]), ctx.dev(cam["P_inv"]),
                           ctx.dev(cam["center"]), sm, S, pts, depth)
    return S.cpu().numpy(), pts.cpu().numpy(), depth.cpu().numpy()


def _depth_of_first_maximum(S, pts, centre):
    k = np.argmax(S, axis=1)                               # the first maximum
    best = pts[np.arange(len(S)), k, :3]
    total = np.zeros(len(S), np.float32)
    for i in range(3):
        d = best[:, i] - np.float32(centre[i])
        total = total + d * d
    return np.sqrt(total)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("NF", [(5, 32), (2, 12)])
@pytest.mark.parametrize("scheme", ["sample_in_range", "sample_in_disparity"])
@pytest.mark.parametrize("kind", KINDS)
def test_k10_points_plane_and_depth(torch, kind, scheme, NF, D):
    N, F = NF
    scene = _scene(kind)
    cam = st.camera_arrays(scene, 0, N)
    ctx = _ctx(scene, D, N, F)
    feats = _features(N, F)
    sm = _sampling(ctx, scheme, kind, cam)
    for n in RAY_COUNTS:
        ridx = st.rays_with_misses(scene, 0, n, seed=D + n)
        S, pts, depth = _k10(torch, ctx, sm, ridx, feats, cam, D)
        assert _same_bits(pts, _k8(torch, ctx, sm, ridx, cam, D))
        assert _same_bits(S, _k9(torch, ctx, sm, ridx, feats, cam, D))
        assert _same_bits(depth, _depth_of_first_maximum(S, pts, cam["center"]))
        missed = pts[:, 0, 3] == 0
        assert np.all(depth[missed] == 0) and np.all(np.isfinite(depth))
        if scheme == "sample_in_range":
            r0, r1 = st.RANGES[kind]
            assert np.all((depth >= r0 - FP32_SLACK) & (depth <= r1 + FP32_SLACK))


# ------------------------------------------------------------------ rn_batch_rays_scheme
def _batch(torch, hip, view, ridx, depth, cams, nbr, patch, N, D, sampling):
    n = len(ridx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")      # noqa: E731
    points = torch.full((n, D, 4), -7.0, device="cuda")
    target = torch.full((n, 4), -7.0, device="cuda")
    centres = torch.full((n, N, D, 2), -7, dtype=torch.int32, device="cuda")
    flags = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    hip.batch_rays(t(view), t(ridx), t(depth), t(cams), t(nbr), patch, points, target, centres, flags,
                   sampling=sampling)
    return tuple(a.cpu().numpy() for a in (points, target, centres, flags))


def _centres_and_crossing(pts, view, cams, nbr, H, W, ph, pw):
    """rn_batch_rays' centres and border flag (tests/batch_truth.py's statement) on given points."""
    n, D = pts.shape[:2]
    N = nbr.shape[1]
    centres = np.zeros((n, N, D, 2), np.int32)
    crossing = np.zeros(n, bool)
    X, Y, Z = pts[..., 0], pts[..., 1], pts[..., 2]
    with np.errstate(all="ignore"):
        for j in range(N):
            P = cams[nbr[view, j]][:, 16:].reshape(n, 3, 4)[:, :, None, :]
            q = [((P[:, i, :, 0] * X + P[:, i, :, 1] * Y) + P[:, i, :, 2] * Z) + P[:, i, :, 3]
                 for i in range(3)]
            x, y = q[0] / q[2], q[1] / q[2]
            cx, cy = bt.to_i32(np.rint(x)), bt.to_i32(np.rint(y))
            centres[:, j, :, 0], centres[:, j, :, 1] = cx, cy
            crossing |= ~bt._inside(x, y, q[2], cx, cy, H, W, ph, pw).all(1)
    return centres, crossing


@pytest.mark.parametrize("D", [5, 33, 70])
@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("scheme", ["sample_in_range", "sample_in_disparity"])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_rays_scheme(torch, kind, scheme, N, D):
    scene = _scene(kind)
    V = scene.n_images
    cams, nbr = bt.tables(scene, N)
    hip = _ctx(scene, D, N, 32)
    bbox = np.asarray(scene.bbox, np.float32).ravel()
    patch = (5, 7)
    rng = np.random.default_rng(D)
    sm = hip.sampling(scheme, st.RANGES[kind], far_from_table=True)
    for n in RAY_COUNTS:
        view = rng.integers(0, V, n).astype(np.int32)
        ridx = rng.integers(0, st.H * st.W, n).astype(np.int32)
        depth = rng.uniform(1.0, 6.0, n).astype(np.float32)
        depth[::7] = 0.0
        points, target, centres, flags = _batch(torch, hip, view, ridx, depth, cams, nbr, patch, N, D, sm)
        if n == 0:
            continue
        # points: K8's with the ray's own view (and that view's far view), bit for bit
        for v in np.unique(view):
            sel = view == v
            cam = dict(P_inv=cams[v, :12].reshape(4, 3), center=cams[v, 12:16])
            far = cams[nbr[v, N - 1]]
            smv = hip.sampling(scheme, st.RANGES[kind], (far[16:], far[:12], far[12:16]))
            assert _same_bits(points[sel], _k8(torch, hip, smv, ridx[sel], cam, D))
        # target as rn_batch_rays states it; centres and flags by its definitions on the new points
        old = bt.batch_rays_f32(view, ridx, depth, cams, nbr, bbox, st.H, st.W, D, patch)
        assert _same_bits(target, old["target"])
        want_c, crossing = _centres_and_crossing(points[..., :3], view, cams, nbr, st.H, st.W, *patch)
        assert np.array_equal(centres, want_c)
        missed = points[:, 0, 3] == 0
        assert not missed.any() or scheme == "sample_in_disparity"
        want_f = (old["flags"] & (bt.NO_DEPTH | bt.TARGET_OUTSIDE)) | missed * bt.MISSES_BOX | \
            crossing * bt.BORDER
        assert np.array_equal(flags, want_f.astype(np.int32))


# ------------------------------------------------------------------ nothing that exists moved
@pytest.mark.parametrize("D", [16, 33, 70])
@pytest.mark.parametrize("NF", [(5, 32), (2, 12)])
def test_bbox_through_the_new_entries_is_the_old_entries(torch, NF, D):
    N, F = NF
    scene = _scene("ring")
    cam = st.camera_arrays(scene, 0, N)
    ctx = _ctx(scene, D, N, F)
    feats = _features(N, F)
    sm = ctx.sampling("sample_in_bbox")
    ridx = st.rays_with_misses(scene, 0, 200, seed=D)
    n = len(ridx)
    d = ctx.dev
    pts_old = torch.zeros((n, D, 4), device="cuda")
    ctx.sample_points(d(ridx), d(cam["P_inv"]), d(cam["center"]), pts_old)
    assert _same_bits(_k8(torch, ctx, sm, ridx, cam, D), pts_old.cpu().numpy())
    S_old = torch.zeros((n, D), device="cuda")
    ctx.mvcnn_similarities(d(ridx), d(feats), d(cam["P"]), d(cam["P_inv"]), d(cam["center"]), S_old)
    assert _same_bits(_k9(torch, ctx, sm, ridx, feats, cam, D), S_old.cpu().numpy())
    S2, p2, z2 = torch.zeros((n, D), device="cuda"), torch.zeros((n, D, 4), device="cuda"), \
        torch.zeros((n,), device="cuda")
    ctx.mvcnn_depth(d(ridx), d(feats), d(cam["P"]), d(cam["P_inv"]), d(cam["center"]), S2, p2, z2)
    S, pts, depth = _k10(torch, ctx, sm, ridx, feats, cam, D)
    assert _same_bits(S, S2.cpu().numpy()) and _same_bits(pts, p2.cpu().numpy())
    assert _same_bits(depth, z2.cpu().numpy())
    if F == 32:
        cams, nbr = bt.tables(scene, N)
        rng = np.random.default_rng(D)
        view = rng.integers(0, scene.n_images, n).astype(np.int32)
        depth_in = rng.uniform(1.0, 6.0, n).astype(np.float32)
        new = _batch(torch, ctx, view, ridx, depth_in, cams, nbr, (5, 7), N, D, sm)
        old = _batch(torch, ctx, view, ridx, depth_in, cams, nbr, (5, 7), N, D, None)
        for a, b in zip(new, old):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------ error paths
def test_invalid_arguments_are_refused_without_a_launch(torch):
    from raynet_amd import _lib
    scene = _scene("ring")
    cam = st.camera_arrays(scene, 0, 2)
    ctx = _ctx(scene, 5, 2, 12)
    lib = ctx.lib
    ridx = ctx.dev(st.rays_with_misses(scene, 0, 8))
    canary = torch.full((8, 5, 4), -7.0, device="cuda")

    def call(sm):
        rc = lib.rn_sample_points_scheme(ctx._h, 8, ctypes.c_void_p(ridx.data_ptr()),
                                         ctypes.c_void_p(ctx.dev(cam["P_inv"]).data_ptr()),
                                         ctypes.c_void_p(ctx.dev(cam["center"]).data_ptr()), sm,
                                         ctypes.c_void_p(canary.data_ptr()), None)
        torch.cuda.synchronize()
        return rc, lib.rn_last_error(ctx._h).decode()
    for r in ((4.0, 2.0), (3.0, 3.0), (0.0, 2.0), (-1.0, 2.0), (1.0, float("inf")), (float("nan"), 2.0)):
        rc, msg = call(ctypes.byref(ctx.sampling("sample_in_range", r)))
        assert rc == -1 and "depth range" in msg, (r, rc, msg)
    sm = ctx.sampling("sample_in_bbox")
    sm.scheme = 7
    rc, msg = call(ctypes.byref(sm))
    assert rc == -1 and "unknown sampling scheme 7" in msg
    rc, msg = call(None)
    assert rc == -1 and "sampling is required" in msg
    assert torch.all(canary == -7.0)                       # nothing was launched
    with pytest.raises(_lib.RaynetHipError, match="unknown sampling scheme"):
        ctx.sample_points_scheme(ridx, ctx.dev(cam["P_inv"]), ctx.dev(cam["center"]), sm, canary)
    # D = 1: no context of that shape exists (rn_create refuses it; the entries check D >= 2 too)
    cfg = _lib.Config()
    cfg.M, cfg.D, cfg.N, cfg.F, cfg.H, cfg.W, cfg.padding = 8, 1, 2, 12, st.H, st.W, PAD
    for i in range(3):
        cfg.grid[i] = 4
        cfg.bbox[i], cfg.bbox[3 + i] = -1.0, 1.0
    h = ctypes.c_void_p()
    assert lib.rn_create(ctypes.byref(cfg), ctypes.byref(h)) == -1 and not h.value
    # n == 0: RN_OK, pointers may be null, nothing is launched -- every entry, both schemes
    for scheme in ("sample_in_range", "sample_in_disparity"):
        sm = ctypes.byref(ctx.sampling(scheme, (2, 4), (np.eye(3, 4), np.eye(4, 3), np.ones(4))))
        assert lib.rn_sample_points_scheme(ctx._h, 0, None, None, None, sm, None, None) == 0
        assert lib.rn_mvcnn_similarities_scheme(ctx._h, 0, None, None, None, None, None, sm, None, None) == 0
        assert lib.rn_mvcnn_depth_scheme(ctx._h, 0, None, None, None, None, None, sm, None, None, None,
                                         None) == 0
        assert lib.rn_batch_rays_scheme(ctx._h, 0, None, None, None, None, 0, None, 0, 0, 0, sm, None,
                                        None, None, None, None) == 0
        # ... and with buffers handed in, none of them is touched
        S = torch.full((8, 5), -7.0, device="cuda")
        depth = torch.full((8,), -7.0, device="cuda")
        P = ctx.dev(cam["P"])
        feats = ctx.dev(_features(2, 12))
        p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
        P_inv, centre = ctx.dev(cam["P_inv"]), ctx.dev(cam["center"])
        assert lib.rn_mvcnn_similarities_scheme(ctx._h, 0, p(ridx), p(feats), p(P), p(P_inv), p(centre),
                                                sm, p(S), None) == 0
        assert lib.rn_mvcnn_depth_scheme(ctx._h, 0, p(ridx), p(feats), p(P), p(P_inv), p(centre), sm,
                                         p(S), p(canary), p(depth), None) == 0
        torch.cuda.synchronize()
        assert torch.all(S == -7.0) and torch.all(canary == -7.0) and torch.all(depth == -7.0)
    # an invalid scheme is refused by the sweep entries too, before anything runs
    bad = ctx.sampling("sample_in_range", (4.0, 2.0))
    assert lib.rn_mvcnn_similarities_scheme(ctx._h, 8, None, None, None, None, None, ctypes.byref(bad),
                                            None, None) == -1
    assert "depth range" in lib.rn_last_error(ctx._h).decode()
    assert lib.rn_mvcnn_depth_scheme(ctx._h, 8, None, None, None, None, None, ctypes.byref(bad), None,
                                     None, None, None) == -1


# ------------------------------------------------------------------ drivers
def test_forward_pass_driver_with_sample_in_range(torch):
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.forward_pass import MultiViewCNNForwardPass
    from raynet_amd.synthetic import make_synthetic_scene
    D, r0, r1 = 16, 2.0, 4.0
    scene, bank = make_synthetic_scene(H=st.H, W=st.W, n_views=5, F=32, padding=PAD)
    gp = GenerationParameters(depth_planes=D, neighbors=4, padding=PAD, depth_range=(r0, r1),
                              sampling_type="sample_points_in_range")
    fp = MultiViewCNNForwardPass(bank, gp, "sample_in_range", scene.image_shape, rays_batch=500)
    maps = list(fp.forward_pass(scene, (0, 2, 1)))
    assert len(maps) == 2
    steps = (np.float64(r0) + np.arange(D) * (r1 - r0) / (D - 1))
    for m in maps:
        assert m.shape == (st.H, st.W) and m.dtype == np.float32
        assert np.all((m >= r0 - FP32_SLACK) & (m <= r1 + FP32_SLACK))
        # the distance of one of the D samples
        assert np.abs(m[..., None] - steps).min(-1).max() <= FP32_SLACK
    assert len({float(v) for v in np.round(maps[0].ravel(), 4)}) > 1


@pytest.mark.parametrize("policy", ["sample_points_in_range", "sample_points_in_disparity"])
def test_one_pretraining_step(torch, policy):
    from raynet_amd.common.generation_parameters import GenerationParameters
    from raynet_amd.models import get_nn
    from raynet_amd.train_network.ray_sampler import RayBatchSampler, SceneBank
    from raynet_amd.train_network.targets import get_target_distribution_factory
    from raynet_amd.train_network.trainer import Trainer
    scene = bt.plane_scene(GOLDEN)
    lo, hi = scene.gt_depth_range

    class Dataset(object):
        n_scenes = 1

        def get_scene(self, i):
            return scene
    gp = GenerationParameters(depth_planes=8, neighbors=4, grid_shape=np.array([32, 32, 16], np.int32),
                              max_number_of_marched_voxels=96, depth_range=(0.8 * float(lo), 1.2 * float(hi)),
                              sampling_type=policy)
    gp.target_distribution_factory = get_target_distribution_factory("dirac")
    sampler = RayBatchSampler(SceneBank(Dataset(), gp), 128, mode="pretrain", seed=3)
    assert sampler.sampling_scheme == policy.replace("sample_points", "sample")
    batch = sampler.next_batch()
    assert len(batch) == 128 and int(batch.flags.abs().sum()) == 0
    points = batch.inputs[5 + 4]
    assert tuple(points.shape) == (128, 8, 4) and bool(torch.all(points[..., 3] == 1))
    torch.manual_seed(0)
    model = get_nn("simple_cnn")(in_channels=3).to("cuda")
    trainer = Trainer(model, "pretrain", 5, None, loss="emd", lr=2e-3,
                      target_distribution_factory=gp.target_distribution_factory)
    loss = trainer.train_step(batch)
    assert np.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
