"""What the accumulator scatter is defined to compute, in plain NumPy, and a census of the routes
k_scatter_box takes on given voxel lists (raynet_amd/csrc/raynet_mrf.inl).  No GPU in here;
tests/test_scatter_truth.py holds every function to hand-made closed forms.

Conventions: `lists` are the rays' voxels as [n][M][3] integers (or packed [n][M] words,
x << 20 | y << 10 | z), `counts` [n] the voxels a ray crossed.  A ray SENDS its first
min(count, M) messages, and only if its count is above 1 (mrf_np.py:300)."""
import numpy as np

# tile shapes of the LDS-box scatter by level: rays, steps, voxels of the LDS box (BoxPolicy)
LEVELS = {0: (128, 32, 4096), 1: (256, 16, 6144)}
SLAB_ROWS, SLAB_STEPS = 64, 16          # what one slab box describes (include/raynet_hip.h)
EMPTY_SLAB = (0x7FFFFFFF, -1)           # k_traverse's entry for a slab no ray emitted a voxel in


def fixed(m):
    """A message as the fixed-point mode sums it: rint(m * 2^32) as int64.  The product is exact
    in float64 (a float32 times a power of two) and ties go to even, as __double2ll_rn rounds
    them.  FINITE messages only: msg_to_fixed's saturation / NaN branch is not restated here
    (k_bp never emits a non-finite message; the parity tests assert that)."""
    m = np.asarray(m)
    assert np.isfinite(m).all()
    return np.rint(m.astype(np.float64) * 2.0 ** 32).astype(np.int64)


def unpack(lists):
    """[n][M][3] int64 from either form of the lists."""
    lists = np.asarray(lists)
    if lists.ndim == 2:
        lists = np.stack([lists >> 20, (lists >> 10) & 1023, lists & 1023], -1)
    return lists.astype(np.int64)


def sending(counts, M):
    """Messages every ray sends: min(count, M), and none at all with a count of 0 or 1."""
    c = np.minimum(np.asarray(counts).astype(np.int64), int(M))
    return np.where(c <= 1, 0, c)


def _pairs(lists, counts):
    """(voxels [P][3], ray [P], step [P]) of every (ray, voxel) pair that is summed."""
    lists = unpack(lists)
    n, M = lists.shape[:2]
    live = np.arange(M)[None, :] < sending(counts, M)[:, None]
    r, i = np.nonzero(live)
    return lists[r, i], r, i


def partial_fixed(msgs, lists, counts, grid):
    """int64 [gx][gy][gz]: the sum of fixed(msgs[r, i]) over i < min(counts[r], M) of the rays
    with counts[r] > 1, at the voxels lists[r, i]."""
    v, r, i = _pairs(lists, counts)
    out = np.zeros(tuple(int(g) for g in grid), np.int64)
    np.add.at(out, (v[:, 0], v[:, 1], v[:, 2]), fixed(np.asarray(msgs)[r, i]))
    return out


def partial_f64(msgs, lists, counts, grid):
    """The same sum in float64 -> (sum, n_v, a_v), each [gx][gy][gz]: n_v the pairs that land on
    a voxel (int64), a_v the sum of their |message|."""
    v, r, i = _pairs(lists, counts)
    at = (v[:, 0], v[:, 1], v[:, 2])
    m = np.asarray(msgs)[r, i].astype(np.float64)
    shape = tuple(int(g) for g in grid)
    total, n_v, a_v = np.zeros(shape), np.zeros(shape, np.int64), np.zeros(shape)
    np.add.at(total, at, m)
    np.add.at(n_v, at, 1)
    np.add.at(a_v, at, np.abs(m))
    return total, n_v, a_v


def brick_index(x, y, z, grid):
    """Offset of voxel (x, y, z) in a resident, 4x4x4-bricked accumulator over `grid` (the
    library's k_occupancy_grid<true> / lin_xyz<true>), in plain integer arithmetic."""
    x, y, z = (np.asarray(a).astype(np.int64) for a in (x, y, z))
    nby, nbz = (int(grid[1]) + 3) // 4, (int(grid[2]) + 3) // 4
    return ((((x >> 2) * nby + (y >> 2)) * nbz + (z >> 2)) << 6) | ((x & 3) << 4) | ((y & 3) << 2) | (z & 3)


def from_bricked(acc, grid):
    """[gx][gy][gz] view (a copy) of a bricked accumulator of any dtype, and the number of
    nonzero entries of `acc` that are no voxel's (the padding of partial bricks)."""
    acc = np.asarray(acc).ravel()
    gx, gy, gz = (int(g) for g in grid)
    X, Y, Z = np.meshgrid(np.arange(gx), np.arange(gy), np.arange(gz), indexing="ij")
    at = brick_index(X, Y, Z, grid)
    stray = int(np.count_nonzero(acc)) - int(np.count_nonzero(acc[at]))
    return acc[at], stray


def slab_table(lists, counts, M):
    """The slab boxes as k_traverse leaves them for rows it wrote itself: int32
    [ceil(n / 64)][ceil(M / 16)][2], per 64 rows and 16 steps the packed min and max corner of
    the voxels those rays have there -- of EVERY ray with a voxel in the slab, also one whose
    single voxel sends nothing; a ray's extremes in a slab are its first and last voxel there (a
    DDA is monotone along every axis, and so are these lists by assumption).  A slab without
    voxels is EMPTY_SLAB."""
    lists = unpack(lists)
    n, M = lists.shape[0], int(M)
    nb, nsl = -(-n // SLAB_ROWS), -(-M // SLAB_STEPS)
    c = np.minimum(np.asarray(counts).astype(np.int64), M)
    table = np.empty((nb, nsl, 2), np.int32)
    table[..., 0], table[..., 1] = EMPTY_SLAB
    for b in range(nb):
        rows = slice(b * SLAB_ROWS, min(n, (b + 1) * SLAB_ROWS))
        for s in range(nsl):
            emitted = np.clip(c[rows] - s * SLAB_STEPS, 0, SLAB_STEPS)
            has = emitted > 0
            if not has.any():
                continue
            rr = np.arange(rows.start, rows.stop)[has]
            first = lists[rr, s * SLAB_STEPS]
            last = lists[rr, s * SLAB_STEPS + emitted[has] - 1]
            lo = np.minimum(first, last).min(0)
            hi = np.maximum(first, last).max(0)
            table[b, s] = ((lo[0] << 20) | (lo[1] << 10) | lo[2], (hi[0] << 20) | (hi[1] << 10) | hi[2])
    return table


def _volume(lo, hi):
    return np.prod(np.maximum(hi - lo + 1, 0), axis=-1)


def census(lists, counts, M, level, slab_table=None):
    """The routes k_scatter_box takes at tile `level` over these rows, per (tile, chunk): tiles of
    RAYS consecutive rows, chunks of STEPS steps below the tile's longest sending ray.

    Without a table a chunk's box is the exact bounding box of its live pairs; one that exceeds
    CAP voxels is redone in quarters of STEPS / 4 steps (each with its own exact box).  With a
    table (int32 [blocks][ceil(M / 16)][2], what HipContext.bind_slab_boxes returns, read back)
    the box is the kernel's merge of the slab boxes -- a 64-row half counts only up to its own
    longest sending ray, an entry with a negative second word is empty -- and an overflowed
    chunk is redone slab by slab.

    -> dict: chunks, overflowed (the kernel's two counters), fit / nofit (quarters or slabs of
    overflowed chunks that fit the LDS box / go to the direct atomics), in_box (chunks -
    overflowed), volume [tiles][chunks per tile] (box volumes, -1 where no chunk is) and
    pieces [(tile, chunk, piece, volume)] of the overflowed chunks."""
    RAYS, STEPS, CAP = LEVELS[level]
    lists = unpack(lists)
    n, M = lists.shape[0], int(M)
    tiles = -(-n // RAYS)
    Mp = -(-M // STEPS) * STEPS
    nch = Mp // STEPS
    send = np.zeros(tiles * RAYS, np.int64)
    send[:n] = sending(counts, M)
    vox = np.zeros((tiles * RAYS, Mp, 3), np.int64)
    vox[:n, :M] = lists[:, :M]
    live = np.arange(Mp)[None, :] < send[:, None]
    BIG = 1 << 30
    lo_e = np.where(live[..., None], vox, BIG)
    hi_e = np.where(live[..., None], vox, -1)
    tile_max = send.reshape(tiles, RAYS).max(1)
    n_chunks = -(-tile_max // STEPS)                       # live chunks per tile
    is_chunk = np.arange(nch)[None, :] < n_chunks[:, None]
    Q = 4
    # exact boxes per (tile, chunk, quarter)
    q_lo = lo_e.reshape(tiles, RAYS, nch, Q, STEPS // Q, 3).min(axis=(1, 4))
    q_hi = hi_e.reshape(tiles, RAYS, nch, Q, STEPS // Q, 3).max(axis=(1, 4))
    pieces = []
    if slab_table is None:
        c_lo, c_hi = q_lo.min(2), q_hi.max(2)
        volume = np.where(is_chunk, _volume(c_lo, c_hi), -1)
        over = volume > CAP
        for t, ch in zip(*np.nonzero(over)):
            for q in range(Q):
                if q_hi[t, ch, q, 0] >= 0:
                    pieces.append((int(t), int(ch), q, int(_volume(q_lo[t, ch, q], q_hi[t, ch, q]))))
    else:
        HB, SL = RAYS // SLAB_ROWS, STEPS // SLAB_STEPS
        nsl = -(-M // SLAB_STEPS)
        tb = np.asarray(slab_table).reshape(-1, nsl, 2).astype(np.int64)
        full = np.empty((tiles * HB, nch * SL, 2), np.int64)
        full[..., 0], full[..., 1] = EMPTY_SLAB
        full[:min(len(tb), tiles * HB), :nsl] = tb[:tiles * HB]
        half_true = send.reshape(tiles, HB, SLAB_ROWS).max(2)                  # [tiles][HB]
        # slab (tile, hb, chunk, sl) is read iff its first step lies below the half's longest ray
        first_step = (np.arange(nch)[:, None] * STEPS + np.arange(SL)[None, :] * SLAB_STEPS)
        read = first_step[None, None] < half_true[:, :, None, None]
        ent = full.reshape(tiles, HB, nch, SL, 2)
        used = read & (ent[..., 1] >= 0)
        s_lo = np.stack([ent[..., 0] >> 20, (ent[..., 0] >> 10) & 1023, ent[..., 0] & 1023], -1)
        s_hi = np.stack([ent[..., 1] >> 20, (ent[..., 1] >> 10) & 1023, ent[..., 1] & 1023], -1)
        s_lo = np.where(used[..., None], s_lo, BIG)
        s_hi = np.where(used[..., None], s_hi, -1)
        c_lo, c_hi = s_lo.min(axis=(1, 3)), s_hi.max(axis=(1, 3))
        volume = np.where(is_chunk & (c_hi[..., 0] >= 0), _volume(c_lo, c_hi), -1)
        over = volume > CAP
        for t, ch in zip(*np.nonzero(over)):
            for hb in range(HB):
                for sl in range(SL):
                    if used[t, hb, ch, sl]:
                        pieces.append((int(t), int(ch), hb * SL + sl,
                                       int(_volume(s_lo[t, hb, ch, sl], s_hi[t, hb, ch, sl]))))
    fit = sum(1 for p in pieces if p[3] <= CAP)
    chunks, overflowed = int(n_chunks.sum()), int(over.sum())
    return dict(chunks=chunks, overflowed=overflowed, in_box=chunks - overflowed, fit=fit,
                nofit=len(pieces) - fit, volume=volume, pieces=pieces)
