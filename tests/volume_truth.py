"""NumPy restatement of the occupancy volume (include/raynet_hip.h: rn_occupancy_grid,
rn_volume_render) -- the truth of tests/test_volume_gpu.py, itself held to
closed forms by tests/test_volume_truth.py.

belief64 is the definition of a belief in float64; render32 is the rendering of one belief grid
along given voxel lists, operation by operation in np.float32 (every operation rounded on its
own, in the kernel's order), vectorised over the rays and sequential along them.
"""
import numpy as np

F = np.float32
LO, HI = 1e-4, float(np.float32(1 - 1e-4))        # occupancy_to_ray's clamp
PLANES = ("depth", "opacity", "expected_depth", "confidence", "median_depth")


def sigmoid64(acc32):
    a = np.asarray(acc32, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a))


def belief64(acc32):
    """clip(1 / (1 + exp(-a)), 1e-4, float32(1 - 1e-4)) in float64, a the fp32 log-odds"""
    return np.clip(sigmoid64(acc32), LO, HI)


def voxel_distance32(voxels, voxel_grid, center):
    """k_depth's depth arithmetic: sqrt(((dx^2 + dy^2) + dz^2)) in fp32 of the voxel's centre
    against the camera centre.  voxels (..., 3) int; voxel_grid [gx][gy][gz][3] f32."""
    vg = np.asarray(voxel_grid, F)
    c = np.asarray(center, F).ravel()
    v = np.asarray(voxels)
    pt = vg[v[..., 0], v[..., 1], v[..., 2]]                       # (..., 3) f32
    d = [(pt[..., i] - c[i]).astype(F) for i in range(3)]
    s = (d[0] * d[0]).astype(F)            # 0 + dx^2 is dx^2
    s = (s + (d[1] * d[1]).astype(F)).astype(F)
    s = (s + (d[2] * d[2]).astype(F)).astype(F)
    return np.sqrt(s).astype(F)


def render32(lists, counts, belief, voxel_grid, center):
    """-> (5, n) float32, the planes of PLANES.  lists (n, M, 3) int32 voxel lists, counts (n,)
    how many entries of each are voxels, belief [gx][gy][gz] f32."""
    lists, counts = np.asarray(lists), np.asarray(counts)
    belief = np.asarray(belief, F)
    n, M = lists.shape[0], lists.shape[1]
    counts = np.minimum(counts, M)
    one, half = F(1), F(0.5)
    T = np.ones(n, F)
    best_w, best_t = np.zeros(n, F), np.zeros(n, F)
    sum_w, sum_wt = np.zeros(n, F), np.zeros(n, F)
    median = np.zeros(n, F)
    have_median = np.zeros(n, bool)
    for i in range(int(counts.max()) if n else 0):
        live = counts > i
        v = np.where(live[:, None], lists[:, i], 0)
        o = belief[v[:, 0], v[:, 1], v[:, 2]]
        t = voxel_distance32(v, voxel_grid, center)
        w = (o * T).astype(F)
        better = live & ((w > best_w) if i else np.ones(n, bool))      # strict >, the first wins
        best_w = np.where(better, w, best_w)
        best_t = np.where(better, t, best_t)
        sum_wt = np.where(live, (sum_wt + (w * t).astype(F)).astype(F), sum_wt)
        sum_w = np.where(live, (sum_w + w).astype(F), sum_w)
        T = np.where(live, (T * (one - o).astype(F)).astype(F), T)
        now = live & ~have_median & (T <= half)
        median = np.where(now, t, median)
        have_median |= now
    with np.errstate(divide="ignore", invalid="ignore"):
        expected = np.where(sum_w > 0, (sum_wt / sum_w).astype(F), F(0))
    opacity = np.where(counts > 0, (one - T).astype(F), F(0))
    return np.stack([best_t, opacity, expected, best_w, median]).astype(F)


# ---- the fixture the CPU and the GPU tests share ------------------------------------------
GRID = (16, 12, 8)
BBOX = (-0.8, -0.6, -0.4, 0.8, 0.6, 0.4)        # cells of 0.1 along every axis
CENTER = (2.5, -1.75, 1.25)                       # a camera outside the box
N_CHORDS, N_ROWS, N_OUTSIDE = 120, 40, 37


def _face_point(rng, face, lo, hi):
    """a random point on face `face` (axis = face // 2, side = face % 2) of the box"""
    p = rng.uniform(lo, hi)
    p[face // 2] = (lo, hi)[face % 2][face // 2]
    return p


def make_segments(seed=7):
    """-> starts, ends (197, 3) f32: 120 chords between points on two different faces of the box
    (the last 20 cut a corner inside one cell, so that counts of 1 occur), 40 axis-parallel rows
    through voxel centres (both directions), 37 segments wholly outside the box."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(BBOX[:3]), np.array(BBOX[3:])
    cell = (hi - lo) / np.array(GRID)
    s, e = [], []
    for k in range(N_CHORDS - 20):
        fa, fb = rng.choice(6, 2, replace=False)
        s.append(_face_point(rng, fa, lo, hi))
        e.append(_face_point(rng, fb, lo, hi))
    for k in range(20):
        # from the face x = lo to the face y = lo, both points inside the corner cell of a z row
        z = lo[2] + (rng.integers(GRID[2]) + 0.5) * cell[2]
        a = np.array([lo[0], lo[1] + rng.uniform(0.2, 0.8) * cell[1], z])
        b = np.array([lo[0] + rng.uniform(0.2, 0.8) * cell[0], lo[1], z])
        s.append(a if k % 2 == 0 else b)
        e.append(b if k % 2 == 0 else a)
    for k in range(N_ROWS):
        axis = (0, 1, 2)[k % 3]
        idx = [rng.integers(g) for g in GRID]
        a = lo + (np.array(idx) + 0.5) * cell
        b = a.copy()
        a[axis], b[axis] = lo[axis], hi[axis]
        s.append(a if k % 2 == 0 else b)
        e.append(b if k % 2 == 0 else a)
    shift = np.array([3.0, 0.0, 0.0])
    for k in range(N_OUTSIDE):
        fa, fb = rng.choice(6, 2, replace=False)
        s.append(_face_point(rng, fa, lo, hi) + shift)
        e.append(_face_point(rng, fb, lo, hi) + shift)
    return (np.ascontiguousarray(np.array(s), dtype=F), np.ascontiguousarray(np.array(e), dtype=F))
