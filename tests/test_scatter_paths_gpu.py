"""Every route of the accumulator scatter (k_scatter_box, k_scatter_slab, k_scatter_direct_fixed
and their launcher) against tests/scatter_truth.py: the fixed-point mode to the bit, the float
mode within the bound of its additions, and the kernel's own counters against a host census of
the routes -- so that a case KNOWS which branch it ran.  Needs a real MI355X: `-m gpu`.

Routes of k_scatter_box per (tile, chunk):
  1   the chunk's box fits the LDS box
  2a  it does not, slab boxes are bound, the slab's box fits     2b  ... the slab's does not
  3a  it does not, no slab boxes, the quarter's box fits          3b  ... the quarter's does not
Scenes are named after the route they are built for: `dense` (1), `medium` (2a / 3a), `sparse`
(2b / 3b); each case asserts from the host census alone, before anything is launched, that the
route it is named after has at least ROUTE_FLOOR pieces.  The scene makers and route_floor() need
no GPU (tests/test_scatter_truth.py runs them on the CPU)."""
import functools

import numpy as np
import pytest

import scatter_truth as T

pytestmark = pytest.mark.gpu

BBOX = np.array([-1, -1, -1, 1, 1, 1], np.float32)
ROUTE_FLOOR = 8

# the pinhole of test_box_scatter_equals_direct_sum over a 32 x 32 image; the knob is how many
# voxels apart neighbouring rays are where they leave the box: name -> (grid, M, spacing)
PINHOLE = {
    "dense": ((48, 48, 48), 96, 0.7),
    "medium": ((96, 96, 48), 96, 1.5),
    "sparse": ((256, 256, 32), 96, 4.0),         # thin: a small accumulator under wide bundles
}
# ... on grids that are no multiple of the 4x4x4 brick, M no multiple of 32 (nor of 16)
PINHOLE_ODD = {
    "dense": ((50, 50, 50), 90, 0.7),
    "medium": ((98, 98, 50), 90, 1.5),
    "sparse": ((254, 254, 30), 90, 4.0),
}
# rows rn_scene_prepare_all writes (view 0 of raynet_amd.synthetic's ring, 32 x 32 pixels); the
# knob is the focal length: name -> (grid, M, focal)
RING = {
    "medium": ((96, 96, 48), 96, 96.0),
    "sparse": ((96, 96, 96), 96, 48.0),
}
RING_SHAPE = dict(D=16, N=2, F=32, H=32, W=32, padding=11)


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def patch_order(H, W, rows=None):
    import torch
    from raynet_amd.forward_pass import tile_order
    idx = tile_order(torch.arange(H * W, dtype=torch.int32), H, W, 16, 16).numpy()
    return idx if rows is None else idx[:rows]


@functools.lru_cache(maxsize=None)
def pinhole_lists(grid, M, spacing, rows=1024, H=32, W=32):
    """-> (lists [rows][M][3] i32, counts [rows] i32) of the oracle's traversal: a camera in front
    of the box, rows in 16 x 16 patch order, neighbouring rays `spacing` voxels apart on the
    box's far face (half of that where they enter)."""
    oracle = _oracle()
    o = oracle.Oracle(M=M, D=8, N=2, F=4, H=H, W=W, padding=3, bbox=BBOX, grid_shape=grid)
    idx = patch_order(H, W, rows)
    x, y = (idx // H).astype(np.float32), (idx % H).astype(np.float32)
    cam = np.array([0.1, -0.2, -3.0], np.float32)
    tgt = np.stack([(x - W / 2 + 0.5) * spacing * 2 / grid[0],
                    (y - H / 2 + 0.5) * spacing * 2 / grid[1],
                    np.ones(len(idx), np.float32)], 1).astype(np.float32)
    d = tgt - cam
    starts = (cam + d * (2.0 / d[:, 2:3])).astype(np.float32)       # plane z = -1
    ends = (cam + d * (4.0 / d[:, 2:3])).astype(np.float32)         # plane z = +1
    lists, counts = o.traversal(starts, ends)
    lists.setflags(write=False)
    counts.setflags(write=False)
    return lists, counts


def ring_cameras_of(focal):
    from raynet_amd.synthetic import ring_cameras
    return ring_cameras(5, RING_SHAPE["H"], RING_SHAPE["W"], focal=focal)


@functools.lru_cache(maxsize=None)
def ring_lists(grid, M, focal):
    """What rn_scene_prepare_all's traversal writes for view 0 of the synthetic ring, by the oracle
    (sample_in_bbox and the DDA are bit-exact with it) -> (lists, counts, ray indices)."""
    oracle = _oracle()
    o = oracle.Oracle(M=M, bbox=BBOX, grid_shape=grid, **RING_SHAPE)
    idx = patch_order(RING_SHAPE["H"], RING_SHAPE["W"])
    cam = ring_cameras_of(focal)[0]
    starts, ends = o.sample(idx, np.asarray(cam.P_pinv, np.float32),
                            np.asarray(cam.center, np.float32).ravel())
    lists, counts = o.traversal(starts, ends)
    for a in (lists, counts, idx):
        a.setflags(write=False)
    return lists, counts, idx


def field_limit_lists():
    """M = 1024 and 300 rays along the long axis of a thin grid, as in test_maximum_sizes_m1024 --
    but 1024 voxels long, not 1000: a DDA's list has at most gx + gy + gz - 2 voxels, 1006 on
    (1000, 4, 4), i.e. 63 chunks of 16 steps and a largest first chunk of 62.  Only rays of more
    than 1008 voxels open the 64th chunk, whose item carries the field's maximum of 63."""
    oracle = _oracle()
    M, grid, n = 1024, (1024, 4, 4), 300
    bbox = np.array([-10, -0.04, -0.04, 10, 0.04, 0.04], np.float32)
    o = oracle.Oracle(M=M, D=8, N=2, F=4, H=4, W=4, padding=3, bbox=bbox, grid_shape=grid)
    rng = np.random.default_rng(2)
    starts = np.c_[-10 * np.ones(n), rng.uniform(-0.03, 0.03, (n, 2))].astype(np.float32)
    ends = np.c_[10 * np.ones(n), rng.uniform(-0.03, 0.03, (n, 2))].astype(np.float32)
    ends[:10, 0] = rng.uniform(-9, 9, 10)             # some shorter rays
    lists, counts = o.traversal(starts, ends)
    return lists, counts, grid, M, bbox


def route_floor(name, c):
    """The condition on a fixture: the host census `c` of a scene named `name` has the routes the
    name promises, ROUTE_FLOOR (tile, chunk) pieces at least."""
    if name == "dense":
        assert c["overflowed"] == 0 and c["in_box"] >= ROUTE_FLOOR, (name, c["chunks"], c["overflowed"])
    elif name == "medium":
        assert c["fit"] >= ROUTE_FLOOR and c["fit"] > c["nofit"], (name, c["fit"], c["nofit"])
    else:
        assert name == "sparse"
        assert c["nofit"] >= ROUTE_FLOOR, (name, c["fit"], c["nofit"])


def columns(counts, M, seed):
    """Peaked Sr columns, as test_bp_single_sweep_against_float64_truth makes them."""
    rng = np.random.default_rng(seed)
    S = np.zeros((len(counts), M), np.float32)
    for r, c in enumerate(np.minimum(counts, M)):
        if c > 0:
            v = rng.random(c) ** 6 + 1e-6
            v[rng.integers(0, c)] += rng.random() * 5
            S[r, :c] = v / v.sum()
    return S


def saturated_accumulator(shape, seed, occupied=0.01):
    """Log-odds up to +-40: free space at -2 .. -40 and a fraction `occupied` of the voxels at
    0 .. +40.  With the peaked columns the messages then span from below 2^-9, where fixed()
    rounds, to k_bp's clamp -- and few are exactly 0 (behind a saturated voxel a ray's
    transmittance, and with it every later message, underflows: an accumulator of +-40
    everywhere leaves 92 % of the messages at exactly 0, and a dropped 0 shows nowhere)."""
    rng = np.random.default_rng(seed)
    free = -(rng.random(shape) * 38 + 2)
    return np.where(rng.random(shape) < occupied, rng.random(shape) * 40, free).astype(np.float32)


def pack(lists):
    return ((lists[..., 0] << 20) | (lists[..., 1] << 10) | lists[..., 2]).astype(np.int32)


# ---------------------------------------------------------------------------------- GPU side
@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU (no CPU fallback exists)"
    from raynet_amd import _lib
    _lib.build()
    return torch


def fresh_context(torch, M, grid, bbox=BBOX, shape=None, **options):
    """A context of its own (the counters and the tile level are per context), options applied."""
    from raynet_amd.hip_implementations.context import HipContext
    from raynet_amd.hip_implementations.options import PathOptions
    shape = shape or dict(D=8, N=2, F=4, H=4, W=4, padding=3)
    ctx = HipContext(M, shape["D"], shape["N"], shape["F"], shape["H"], shape["W"],
                     shape["padding"], bbox, grid)
    ctx.set_voxel_grid(torch.from_numpy(_oracle().voxel_grid_centers(np.asarray(bbox, np.float32), grid)).cuda())
    ctx.set_options(PathOptions(**options))
    return ctx


def pinned(level):
    return dict(box_level=level, box_pin=True)


def sweeps(torch, ctx, fixed, Sr, vox, rvc, how_many=2, seed=7, occupied=0.01):
    """`how_many` BP sweeps over patch-ordered packed rows, each into a zeroed partial, the device
    idle in between (so that the counters of sweep k are on the host when sweep k + 1 is
    launched) -> [(partial as NumPy, messages as NumPy)] per sweep."""
    G = ctx.acc_size()
    acc_in = torch.from_numpy(saturated_accumulator(G, seed, occupied)).cuda()
    msgs = torch.zeros((len(rvc), ctx.M), device="cuda")
    out = []
    for k in range(how_many):
        part = torch.zeros((G,), dtype=torch.int64 if fixed else torch.float32, device="cuda")
        run = ctx.scene_bp_sweep_fixed if fixed else ctx.scene_bp_sweep
        run(Sr, vox, rvc, acc_in, msgs, part, first_sweep=(k == 0), patch_rows=True)
        torch.cuda.synchronize()
        out.append((part.cpu().numpy(), msgs.cpu().numpy()))
    return out


def assert_messages_span(msgs, lists, counts, most_zero=0.1):
    """The fixture is worth its name: messages from below 2^-9 to the clamp, few exact zeros."""
    live = np.arange(msgs.shape[1])[None, :] < T.sending(counts, msgs.shape[1])[:, None]
    m = np.abs(msgs[live])
    print("messages: %d, |m| in [%g, %g], %.3f exactly 0, %.3f below 2^-9" % (
        m.size, m.min(), m.max(), (m == 0).mean(), (m < 2.0 ** -9).mean()))
    assert np.isfinite(m).all() and m.min() < 2.0 ** -9 and m.max() > 8.0, (m.min(), m.max())
    assert (m == 0).mean() <= most_zero


def assert_fixed(part, msgs, lists, counts, grid, what=""):
    """The bricked int64 partial IS partial_fixed of these messages."""
    got, stray = T.from_bricked(part, grid)
    truth = T.partial_fixed(msgs, lists, counts, grid)
    bad = np.argwhere(got != truth)
    print("%s: %d voxels hit, %d differ, %d stray" % (what, np.count_nonzero(truth), len(bad), stray))
    assert stray == 0, "%s: %d nonzero entries outside the grid's voxels" % (what, stray)
    assert len(bad) == 0, "%s: %d voxels differ; first %s: got %d, truth %d (difference %g messages' worth)" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], truth[tuple(bad[0])],
        (got[tuple(bad[0])] - truth[tuple(bad[0])]) / 2.0 ** 32)


def assert_float(got, msgs, lists, counts, grid, what=""):
    """A float partial [gx][gy][gz] within the bound of ANY order of n_v fp32 additions plus one
    rounding of a box sum: 1.01 (n_v + 1) 2^-24 a_v per voxel; exactly 0 where no pair lands."""
    truth, n_v, a_v = T.partial_f64(msgs, lists, counts, grid)
    err = np.abs(got.astype(np.float64) - truth)
    bound = 1.01 * (n_v + 1) * 2.0 ** -24 * a_v
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)
    w = np.unravel_index(ratio.argmax(), ratio.shape)
    print("%s: worst error / bound %.3g at %s (n_v %d)" % (what, ratio.max(), w, n_v[w]))
    assert np.all(got[n_v == 0] == 0), "%s: a voxel no pair touches is not 0" % what
    assert np.all(err <= bound), "%s: voxel %s: got %r, truth %r, bound %g, n_v %d" % (
        what, w, got[w], truth[w], bound[w], n_v[w])


def assert_counters(ctx, level, c, what=""):
    """scatter_state() after the second sweep: the counters of the first."""
    state = ctx.scatter_state()
    print("%s: state %s, census chunks %d overflowed %d fit %d nofit %d" % (
        what, state, c["chunks"], c["overflowed"], c["fit"], c["nofit"]))
    assert state == (level, c["chunks"], c["overflowed"]), (what, state, c["chunks"], c["overflowed"])


def upload(torch, lists, counts, M, seed):
    return (torch.from_numpy(columns(counts, M, seed)).cuda(), torch.from_numpy(pack(lists)).cuda(),
            torch.from_numpy(counts.copy()).cuda())


# ----------------------------------------------------------- 1. fixed point, packed, host lists
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("scene,rows", [("dense", 1024), ("medium", 1024), ("sparse", 1024),
                                        ("medium", 1000)])
def test_fixed_point_on_host_made_lists(torch, scene, rows, level):
    """Routes 1, 3a and 3b of both tile shapes, and k_scatter_direct_fixed (level 2), on lists
    the oracle made (no slab boxes exist for them): the int64 partial equals partial_fixed bit
    for bit, and the kernel counted the chunks and overflows the census counts.  1000 rows: the
    last tile is ragged."""
    grid, M, spacing = PINHOLE[scene]
    lists, counts = pinhole_lists(grid, M, spacing, rows)
    c = None
    if level < 2:
        c = T.census(lists, counts, M, level)
        route_floor(scene, c)
    ctx = fresh_context(torch, M, grid, **pinned(level))
    Sr, vox, rvc = upload(torch, lists, counts, M, seed=10 + level)
    runs = sweeps(torch, ctx, True, Sr, vox, rvc)
    if level < 2:
        assert_counters(ctx, level, c, "%s L%d" % (scene, level))
    else:
        assert ctx.scatter_state()[0] == 2
    assert_messages_span(runs[0][1], lists, counts)
    for k, (part, msgs) in enumerate(runs):
        assert_fixed(part, msgs, lists, counts, grid, "%s L%d sweep %d" % (scene, level, k + 1))


# ----------------------------------------------------------- 2. fixed point with slab boxes
def prepared_rows(torch, scene, level):
    """View 0 of the synthetic ring through rn_scene_prepare_all into a list buffer bound with
    bind_slab_boxes -> (ctx, Sr, vox, rvc, table tensor, lists, counts).  Asserts that the lists
    are the oracle's and the table is what scatter_truth.slab_table says the traversal leaves,
    and (before any scatter is launched) the route floor on that host-made table."""
    from raynet_amd.synthetic import make_synthetic_scene
    grid, M, focal = RING[scene]
    sh = RING_SHAPE
    lists, counts, idx = ring_lists(grid, M, focal)
    host_table = T.slab_table(lists, counts, M)
    route_floor(scene, T.census(lists, counts, M, level, host_table))
    if scene == "medium":       # route 2a alone: nothing of this scene takes the direct atomics
        assert T.census(lists, counts, M, level, host_table)["nofit"] == 0
    synth, bank = make_synthetic_scene(H=sh["H"], W=sh["W"], n_views=5, F=sh["F"],
                                       padding=sh["padding"], focal=focal)
    ctx = fresh_context(torch, M, grid, shape=sh, **pinned(level))
    n, N = len(idx), sh["N"]
    views = (0, 1)
    maps = [bank.view_features(synth, v) for v in views]
    table_of_maps = torch.tensor([[m.data_ptr() for m in maps]], dtype=torch.int64).cuda()
    cam = np.zeros((1, 12 * N + 16), np.float32)
    cam[0, :12 * N] = np.array([synth.get_image(v).camera.P for v in views], np.float32).ravel()
    cam[0, 12 * N:12 * N + 12] = np.asarray(synth.get_image(0).camera.P_pinv, np.float32).ravel()
    cam[0, 12 * N + 12:] = np.asarray(synth.get_image(0).camera.center, np.float32).ravel()
    vox = torch.zeros((n, M), dtype=torch.int32, device="cuda")
    rvc = torch.zeros((n,), dtype=torch.int32, device="cuda")
    Sr = torch.zeros((n, M), device="cuda")
    table = ctx.bind_slab_boxes(vox)
    table.fill_(-7)             # (nothing is to be read that the traversal did not write)
    ctx.scene_prepare_all(1, n, torch.from_numpy(idx.copy()).cuda(), table_of_maps,
                          torch.from_numpy(cam).cuda(), vox, rvc, Sr)
    torch.cuda.synchronize()
    ctx._keep = (maps, synth, bank)
    # k_traverse is bit-exact with the oracle: the census tuned on the host is this run's
    assert np.array_equal(rvc.cpu().numpy(), counts)
    live = np.arange(M)[None, :] < np.minimum(counts, M)[:, None]
    assert np.array_equal(vox.cpu().numpy()[live], pack(lists)[live])
    got_table = table.cpu().numpy().reshape(host_table.shape)
    written = host_table[..., 1] >= 0
    assert np.array_equal(got_table[written], host_table[written])
    Sr.copy_(torch.from_numpy(columns(counts, M, seed=20 + level)))
    return ctx, Sr, vox, rvc, table, lists, counts


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("scene", ["medium", "sparse"])
def test_fixed_point_with_slab_boxes(torch, scene, level):
    """Routes 2a (medium) and 2b (sparse): rows rn_scene_prepare_all wrote, their slab boxes
    bound.  Same integers; the kernel's overflow count is the census of the read-back table and
    no less than the exact-box census; and with the table unbound (routes 3a / 3b on the same
    rows) the integers are the same."""
    grid, M, _ = RING[scene]
    ctx, Sr, vox, rvc, table, lists, counts = prepared_rows(torch, scene, level)
    c = T.census(lists, counts, M, level, table.cpu().numpy())
    exact = T.census(lists, counts, M, level)
    assert c["overflowed"] >= exact["overflowed"] and c["chunks"] == exact["chunks"]
    runs = sweeps(torch, ctx, True, Sr, vox, rvc)
    assert_counters(ctx, level, c, "%s slab boxes L%d" % (scene, level))
    assert_messages_span(runs[0][1], lists, counts)
    for k, (part, msgs) in enumerate(runs):
        assert_fixed(part, msgs, lists, counts, grid, "%s slab boxes L%d sweep %d" % (scene, level, k + 1))
    # the same rows with the table unbound: routes 3a / 3b, the exact boxes' counters
    ctx.bind_slab_boxes(None)
    runs2 = sweeps(torch, ctx, True, Sr, vox, rvc)
    assert_counters(ctx, level, exact, "%s unbound L%d" % (scene, level))
    for k, (part, msgs) in enumerate(runs2):
        assert np.array_equal(msgs, runs[k][1])
        assert np.array_equal(part, runs[k][0])


# ----------------------------------------------------------- 3. the work list
def assert_items(items, level, one_chunk_each):
    """The list the kernel is about to walk is of the kind the case is named after."""
    it = items.cpu().numpy()
    first, cn = (it >> 6) & 63, it & 63
    if one_chunk_each:
        assert (cn == 1).all() and (first > 0).any()
    else:
        assert (cn > 1).any()
    return first


@pytest.mark.parametrize("target", [4096, 4], ids=["chunk-per-item", "chunks-per-item"])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("source", ["host", "prepared"])
def test_fixed_point_through_the_work_list(torch, source, level, target):
    """The medium scenes again with rn_scene_bind_scatter_items: one chunk per item (items that
    start at a chunk > 0) and several chunks per item.  Same integers, same counters."""
    if source == "host":
        grid, M, spacing = PINHOLE["medium"]
        lists, counts = pinhole_lists(grid, M, spacing)
        c = T.census(lists, counts, M, level)
        route_floor("medium", c)
        ctx = fresh_context(torch, M, grid, **pinned(level))
        Sr, vox, rvc = upload(torch, lists, counts, M, seed=30 + level)
    else:
        grid, M, _ = RING["medium"]
        ctx, Sr, vox, rvc, table, lists, counts = prepared_rows(torch, "medium", level)
        c = T.census(lists, counts, M, level, table.cpu().numpy())
    items = ctx.bind_scatter_items(vox, rvc, level=level, target_items=target)
    assert items is not None and ctx.scatter_items_bound(items)
    assert_items(items, level, target == 4096)
    runs = sweeps(torch, ctx, True, Sr, vox, rvc)
    assert ctx.scatter_items_bound(items)           # (the sweeps did not drop it)
    assert_counters(ctx, level, c, "%s items L%d" % (source, level))
    for k, (part, msgs) in enumerate(runs):
        assert_fixed(part, msgs, lists, counts, grid, "%s items L%d sweep %d" % (source, level, k + 1))


@pytest.mark.parametrize("level", [0, 1])
def test_work_list_at_the_field_limit(torch, level):
    """M = 1024: an item's 6-bit first-chunk field reaches 63 on 16-step tiles (31 on 32-step
    ones), one chunk per item."""
    lists, counts, grid, M, bbox = field_limit_lists()
    assert counts.max() >= 1000
    c = T.census(lists, counts, M, level)
    ctx = fresh_context(torch, M, grid, bbox=bbox, **pinned(level))
    Sr, vox, rvc = upload(torch, lists, counts, M, seed=40 + level)
    items = ctx.bind_scatter_items(vox, rvc, level=level, target_items=1 << 20)
    first = assert_items(items, level, True)
    assert first.max() == (31 if level == 0 else 63)
    runs = sweeps(torch, ctx, True, Sr, vox, rvc, occupied=0.001)    # (long rays: keep them alive)
    assert_counters(ctx, level, c, "field limit L%d" % level)
    steps = T.LEVELS[level][1]
    assert np.count_nonzero(runs[0][1][:, int(first.max()) * steps:]) > 100     # the last item sums something
    for k, (part, msgs) in enumerate(runs):
        assert_fixed(part, msgs, lists, counts, grid, "field limit L%d sweep %d" % (level, k + 1))


# ----------------------------------------------------------- 4. float, packed
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("scene", ["dense", "medium", "sparse"])
def test_float_packed(torch, scene, level):
    """The float mode (doubles in LDS, float atomics on the accumulator; level 2: k_scatter_slab's
    128-bit load path) on the same routes, within the bound of its additions."""
    grid, M, spacing = PINHOLE[scene]
    lists, counts = pinhole_lists(grid, M, spacing)
    c = None
    if level < 2:
        c = T.census(lists, counts, M, level)
        route_floor(scene, c)
    ctx = fresh_context(torch, M, grid, **pinned(level))
    Sr, vox, rvc = upload(torch, lists, counts, M, seed=50 + level)
    runs = sweeps(torch, ctx, False, Sr, vox, rvc)
    if level < 2:
        assert_counters(ctx, level, c, "float %s L%d" % (scene, level))
    for k, (part, msgs) in enumerate(runs):
        got, stray = T.from_bricked(part, grid)
        assert stray == 0
        assert_float(got, msgs, lists, counts, grid, "float %s L%d sweep %d" % (scene, level, k + 1))


@pytest.mark.parametrize("level", [0, 1])
def test_float_packed_with_slab_boxes(torch, level):
    grid, M, _ = RING["medium"]
    ctx, Sr, vox, rvc, table, lists, counts = prepared_rows(torch, "medium", level)
    c = T.census(lists, counts, M, level, table.cpu().numpy())
    runs = sweeps(torch, ctx, False, Sr, vox, rvc)
    assert_counters(ctx, level, c, "float slab boxes L%d" % level)
    for k, (part, msgs) in enumerate(runs):
        got, stray = T.from_bricked(part, grid)
        assert stray == 0
        assert_float(got, msgs, lists, counts, grid, "float slab boxes L%d sweep %d" % (level, k + 1))


# ----------------------------------------------------------- 5. float, unpacked
@pytest.mark.parametrize("mode", ["box-L0", "box-L1", "slab"])
@pytest.mark.parametrize("scene", ["dense", "medium", "sparse"])
def test_float_unpacked(torch, scene, mode):
    """rn_bp_sweep on [n][M][3] lists into a [gx][gy][gz] accumulator: k_scatter_box<PACKED =
    false> (scatter_mode 2, both tile shapes) and k_scatter_slab<false> (scatter_mode 0).  The
    grid is no multiple of 4 and M none of 32: the slab scatter's generic load path, chunks that
    end inside a tile's steps."""
    grid, M, spacing = PINHOLE_ODD[scene]
    assert any(g % 4 for g in grid) and M % 32 and M % 16
    lists, counts = pinhole_lists(grid, M, spacing)
    level = {"box-L0": 0, "box-L1": 1, "slab": 2}[mode]
    c = None
    if level < 2:
        c = T.census(lists, counts, M, level)
        route_floor(scene, c)
        ctx = fresh_context(torch, M, grid, scatter_mode=2, **pinned(level))
    else:
        ctx = fresh_context(torch, M, grid, scatter_mode=0)
    Sr = torch.from_numpy(columns(counts, M, seed=61 + level)).cuda()
    rvi = torch.from_numpy(lists.copy()).cuda()
    rvc = torch.from_numpy(counts.copy()).cuda()
    acc_in = torch.from_numpy(saturated_accumulator(grid, 60 + level)).cuda()
    msgs = torch.zeros((len(counts), M), device="cuda")
    runs = []
    for k in range(2):
        acc_out = torch.zeros(grid, device="cuda")
        ctx.bp_sweep(Sr, rvi, rvc, acc_in, None if k == 0 else msgs, acc_out, msgs)
        torch.cuda.synchronize()
        runs.append((acc_out.cpu().numpy(), msgs.cpu().numpy()))
    if level < 2:
        assert_counters(ctx, level, c, "unpacked %s %s" % (scene, mode))
    assert_messages_span(runs[0][1], lists, counts)
    for k, (got, m) in enumerate(runs):
        assert_float(got, m, lists, counts, grid, "unpacked %s %s sweep %d" % (scene, mode, k + 1))


# ----------------------------------------------------------- 6. the two-stream split
def test_fixed_point_across_the_two_stream_split(torch):
    """65,536 + 128 patch-ordered rows at level 1: the launcher cuts them at a multiple of 256 and
    scatters the halves on two streams into one partial.  Same integers, every chunk counted."""
    grid, M, rows, H, W = (96, 96, 48), 96, 65536 + 128, 256, 257
    lists, counts = pinhole_lists(grid, M, 0.3, rows, H, W)
    ctx = fresh_context(torch, M, grid, **pinned(1))
    assert ctx.get_options()["overlap"] == 2           # the default: split at level 1
    Sr, vox, rvc = upload(torch, lists, counts, M, seed=70)
    runs = sweeps(torch, ctx, True, Sr, vox, rvc)
    send = np.zeros(-(-rows // 256) * 256, np.int64)
    send[:rows] = T.sending(counts, M)
    chunks = int((-(-send.reshape(-1, 256).max(1) // 16)).sum())
    state = ctx.scatter_state()
    assert state[:2] == (1, chunks), (state, chunks)
    part, msgs = runs[0]
    assert_fixed(part, msgs, lists, counts, grid, "two streams")
    assert_fixed(runs[1][0], runs[1][1], lists, counts, grid, "two streams, sweep 2")
