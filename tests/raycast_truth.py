"""NumPy fp32 brute-force restatement of the ray / mesh first intersection (the semantics of
raynet_amd/mesh.py) -- the truth the GPU kernels are held to bit for
bit, and which tests/test_raycast_reference.py pins to the reference's own golden.

For one ray (o, dst), fp32 throughout, every operation rounded on its own:
  ray = (dst - o) / sqrt(((dx^2 + dy^2) + dz^2));
  per triangle, fast_ray_triangles_intersection's order (raynet/utils/fast_utils.pyx:47-117):
  e1, e2, pvec = ray x e2, det = e1.pvec, reject -1e-6 < det < 1e-6, inv = 1/det,
  u = (o - p0).pvec * inv, reject u < 0 or u > 1, qvec = (o - p0) x e1, v = ray.qvec * inv,
  reject v < 0 or u + v > 1, t = e2.qvec * inv, hit = o + t*ray;
  only t >= 0 counts; the winner has the smallest key ((hx-ox)^2 + (hy-oy)^2) + (hz-oz)^2,
  the lowest triangle index on equal keys (np.argmin over candidates in index order).
"""
import numpy as np

F = np.float32
EPS = F(1e-6)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def normalised_rays(o, dst):
    """[R, 3] f32 unit directions, the reference's arithmetic."""
    r = (np.asarray(dst, F) - np.asarray(o, F)).astype(F)
    norm = np.sqrt(_dot(r[:, 0], r[:, 1], r[:, 2], r[:, 0], r[:, 1], r[:, 2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (r / norm[:, None]).astype(F)


def _test(o, ray, tri):
    """Rays [R] x triangles [T] -> (key [R, T] f32 with inf where rejected, hit xyz)."""
    ox, oy, oz = (o[:, k:k + 1] for k in range(3))
    rx, ry, rz = (ray[:, k:k + 1] for k in range(3))
    p0x, p0y, p0z = (tri[None, :, k] for k in range(3))
    e1x, e1y, e1z = (tri[None, :, 3 + k] - tri[None, :, k] for k in range(3))
    e2x, e2y, e2z = (tri[None, :, 6 + k] - tri[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        px, py, pz = ry * e2z - rz * e2y, rz * e2x - rx * e2z, rx * e2y - ry * e2x
        det = _dot(e1x, e1y, e1z, px, py, pz)
        ok = ~((-EPS < det) & (det < EPS))
        inv = F(1) / det
        tx, ty, tz = ox - p0x, oy - p0y, oz - p0z
        u = _dot(tx, ty, tz, px, py, pz) * inv
        ok &= ~((u < 0) | (u > 1))
        qx, qy, qz = ty * e1z - tz * e1y, tz * e1x - tx * e1z, tx * e1y - ty * e1x
        v = _dot(rx, ry, rz, qx, qy, qz) * inv
        ok &= ~((v < 0) | (u + v > 1))
        t = _dot(e2x, e2y, e2z, qx, qy, qz) * inv
        ok &= t >= 0
        hx, hy, hz = ox + t * rx, oy + t * ry, oz + t * rz
        dx, dy, dz = hx - ox, hy - oy, hz - oz
        key = _dot(dx, dy, dz, dx, dy, dz)
        ok &= key < np.inf                  # (NaN keys never win)
    key = np.where(ok, key, F(np.inf)).astype(F)
    return key, hx, hy, hz


def first_hits(origins, destinations, triangles, candidates=None, chunk=1 << 22):
    """(points [R, 3] f32, triangle [R] int32 (-1: miss)) by brute force over all triangles,
    or over `candidates[r]` (ascending triangle indices) where given."""
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    d = np.ascontiguousarray(destinations, F).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, F).reshape(-1, 9)
    ray = normalised_rays(o, d)
    R = len(o)
    points = np.zeros((R, 3), F)
    idx = np.full((R,), -1, np.int32)
    if candidates is not None:
        for r in range(R):
            c = np.asarray(candidates[r], np.int64)
            if len(c) == 0:
                continue
            key, hx, hy, hz = _test(o[r:r + 1], ray[r:r + 1], tri[c])
            j = int(np.argmin(key[0]))
            if key[0, j] < np.inf:
                idx[r] = c[j]
                points[r] = (hx[0, j], hy[0, j], hz[0, j])
        return points, idx
    step = max(1, chunk // max(1, len(tri)))
    for a in range(0, R, step):
        b = min(R, a + step)
        key, hx, hy, hz = _test(o[a:b], ray[a:b], tri)
        j = np.argmin(key, axis=1)
        rows = np.arange(b - a)
        hit = key[rows, j] < np.inf
        idx[a:b][hit] = j[hit]
        pts = np.stack([hx[rows, j], hy[rows, j], hz[rows, j]], axis=1)
        points[a:b][hit] = pts[hit]
    return points, idx


def culled_candidates(origins, destinations, triangles, block=64, super_block=4096, pad=1e-3):
    """Per ray, the ascending indices of the triangles in blocks of `block` (consecutive in the
    Morton order of their centroids) whose float64 box, widened by `pad` times the mesh's
    scale, meets the ray's line at t >= -pad.
    For well-conditioned meshes (every hit lies within rounding of its triangle) no winner is
    ever culled; the exact test then runs on these triangles only (large meshes)."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = normalised_rays(origins, destinations).astype(np.float64)
    tri = np.asarray(triangles, np.float64).reshape(-1, 3, 3)
    T = len(tri)
    # blocks of triangles that lie close together: Morton order of the centroids
    cen = tri.mean(axis=1)
    q = ((cen - cen.min(0)) / max(float((cen.max(0) - cen.min(0)).max()), 1e-30) * 1023
         ).astype(np.int64)
    code = np.zeros(T, np.int64)
    for b in range(10):
        for k in range(3):
            code |= ((q[:, k] >> b) & 1) << (3 * b + 2 - k)
    perm = np.argsort(code, kind="stable")
    tri = tri[perm]
    lo_t, hi_t = tri.min(axis=1), tri.max(axis=1)
    scale = float(np.abs(np.concatenate([lo_t, hi_t])).max()) + 1.0
    m = pad * scale

    def boxes(size):
        nb = (T + size - 1) // size
        lo = np.full((nb, 3), np.inf)
        hi = np.full((nb, 3), -np.inf)
        np.minimum.at(lo, np.arange(T) // size, lo_t)
        np.maximum.at(hi, np.arange(T) // size, hi_t)
        return lo - m, hi + m

    def meets(oo, dd, lo, hi):
        with np.errstate(all="ignore"):
            inv = 1.0 / dd
            t0 = (lo[None] - oo[:, None]) * inv[:, None]
            t1 = (hi[None] - oo[:, None]) * inv[:, None]
        tmin = np.fmin(t0, t1)
        tmax = np.fmax(t0, t1)
        # an axis the ray runs parallel to: inside the slab or not at all
        par = (dd == 0)[:, None, :]
        inside = (oo[:, None] >= lo[None]) & (oo[:, None] <= hi[None])
        tmin = np.where(par, np.where(inside, -np.inf, np.inf), tmin)
        tmax = np.where(par, np.where(inside, np.inf, -np.inf), tmax)
        tn, tf = np.nanmax(tmin, axis=2), np.nanmin(tmax, axis=2)
        return (tn <= tf) & (tf >= -m)

    slo, shi = boxes(super_block)
    blo, bhi = boxes(block)
    per_super = super_block // block
    out = []
    for a in range(0, len(o), 256):
        sm = meets(o[a:a + 256], d[a:a + 256], slo, shi)
        for r in range(sm.shape[0]):
            sb = np.nonzero(sm[r])[0]
            bl = (sb[:, None] * per_super + np.arange(per_super)[None]).reshape(-1)
            bl = bl[bl < len(blo)]
            hit = bl[meets(o[a + r:a + r + 1], d[a + r:a + r + 1], blo[bl], bhi[bl])[0]]
            c = (hit[:, None] * block + np.arange(block)[None]).reshape(-1)
            out.append(np.sort(perm[c[c < T]]))
    return out


def pixel_rays(P_pinv, center, us, vs):
    """Origins and destinations of pixel rays (raynet_amd.mesh.pixel_destinations'
    convention, restated): float64 products of the fp32 P_pinv rounded once to fp32."""
    P = np.asarray(P_pinv, F).astype(np.float64).reshape(4, 3)
    u = np.asarray(us, np.float64)
    v = np.asarray(vs, np.float64)
    r = [(P[k, 0] * u + P[k, 1] * v) + P[k, 2] for k in range(4)]
    dst = np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], axis=1).astype(F)
    o = np.broadcast_to(np.asarray(center, F).reshape(-1)[:3], dst.shape).copy()
    return o, dst


def depths(points, idx, center):
    """float64 distance of each hit to the centre (geometry.distance), NaN on a miss."""
    c = np.asarray(center, F).reshape(-1)[:3].astype(np.float64)
    dd = points.astype(np.float64) - c
    out = np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
    out[idx < 0] = np.nan
    return out
