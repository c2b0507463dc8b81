"""The truth the surface queries are held to (tests/surface_truth.py) is sound: its two
independent restatements of the distance of a point to a triangle agree, on ordinary meshes
and on triangles collapsed to a segment or a point; the sampler's restated hash is uniform."""
import numpy as np

import surface_truth as truth

F = np.float32


def _soup(rng, n=600):
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.normal(0, 0.15, (n, 3, 3))).reshape(n, 9).astype(F)


def _queries(rng, tri, n=150):
    a, b, c = truth.file_vertices(tri)
    V = np.concatenate([a, b, c])
    lo, hi = V.min(0), V.max(0)
    ext = float((hi - lo).max())
    k = rng.integers(0, len(tri), n)
    bary = rng.dirichlet([1, 1, 1], n)
    on = bary[:, :1] * a[k] + bary[:, 1:2] * b[k] + bary[:, 2:] * c[k]
    Q = [(lo + hi) / 2 + rng.uniform(-1.5, 1.5, (n, 3)) * (hi - lo), on,
         on + rng.normal(0, 0.01 * ext, (n, 3)), a[k], (a[k] + b[k]) / 2, (a[k] + b[k] + c[k]) / 3,
         a[k] + 2 * (b[k] - a[k]), a[k] - 0.5 * (b[k] - a[k]) - 0.7 * (c[k] - a[k]),
         (lo + hi) / 2 + rng.normal(0, 1, (20, 3)) * 1e3 * ext]
    return np.concatenate(Q), ext


def _both(Q, tri):
    a, b, c = truth.file_vertices(tri)
    d1, _ = truth.brute_force(Q, a, b, c, truth.dist_ericson)
    d2, _ = truth.brute_force(Q, a, b, c, truth.dist_segments_plane)
    return d1, d2


def test_the_two_restatements_agree_on_a_soup_and_a_city():
    from raynet_amd.synthetic import make_box_city
    rng = np.random.default_rng(5)
    for tri in (_soup(rng), make_box_city(3000, seed=3000)):
        Q, ext = _queries(rng, tri)
        d1, d2 = _both(Q, tri)
        assert np.isfinite(d1).all() and np.isfinite(d2).all()
        scale = ext + np.abs(Q).max(1)
        err = np.abs(d1 - d2) / scale
        print("%d triangles: max |ericson - segments/plane| = %.3g of (extent + |q|)"
              % (len(tri), err.max()))
        assert (err <= 1e-12).all()
        # a point of the surface is at distance ~0 of it; a far point is not
        n = 150
        assert (d1[n:2 * n] <= 1e-12 * ext).all() and d1[-1] > ext
        # the culled brute force of the GPU tests is the brute force
        a, b, c = truth.file_vertices(tri)
        d3, i3 = truth.brute_force_culled(Q, a, b, c)
        assert np.array_equal(d3, d1)
        assert np.array_equal(truth.dist_ericson(Q, a[i3], b[i3], c[i3]), d1)


def test_exactly_degenerate_triangles_are_their_segment_or_point():
    rng = np.random.default_rng(6)
    p = rng.uniform(-1, 1, (40, 3, 3)).astype(F)
    seg = []
    for k, t in enumerate(p):
        t = t.copy()
        t[[2, 0, 1][k % 3]] = t[[1, 1, 2][k % 3]]          # two vertices coincide
        seg.append(t)
    # three distinct, exactly collinear vertices (exact in fp32 and in the cross products)
    seg.append(np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], F))
    seg.append(np.array([[0.5, 0.25, -1], [0.5, 0.25, 2], [0.5, 0.25, 0.5]], F))
    seg = np.array(seg)
    pts = np.repeat(rng.uniform(-1, 1, (10, 1, 3)).astype(F), 3, axis=1)
    Q = rng.uniform(-3, 3, (400, 3))
    for tris, kind in ((seg, "segment"), (pts, "point")):
        a, b, c = truth.file_vertices(tris.reshape(-1, 9))
        assert (truth.areas(tris.reshape(-1, 9)) == 0).all()
        d1 = truth.dist_ericson(Q[:, None], a[None], b[None], c[None])
        d2 = truth.dist_segments_plane(Q[:, None], a[None], b[None], c[None])
        assert np.isfinite(d1).all() and np.isfinite(d2).all()
        assert (np.abs(d1 - d2) <= 1e-12 * 6).all(), kind
        if kind == "point":
            want = np.sqrt(((Q[:, None] - a[None]) ** 2).sum(-1))
            assert (np.abs(d1 - want) <= 1e-12 * 6).all()
        else:
            # the hull of the three vertices: the longest of the three segments
            ends = [(a, b), (b, c), (c, a)]
            want = np.min([truth._dist_segment(Q[:, None], x[None], y[None]) for x, y in ends], 0)
            assert (np.abs(d1 - want) <= 1e-12 * 6).all()


def test_restated_hash_is_deterministic_and_uniform():
    r = truth.uniforms(0, 30000)
    assert r.shape == (30000, 3) and (r >= 0).all() and (r < 1).all()
    assert np.array_equal(r, truth.uniforms(0, 30000))
    assert not np.array_equal(r, truth.uniforms(1, 30000))
    assert np.abs(r.mean(0) - 0.5).max() < 0.01          # 5.8 standard errors
    # mix64 against splitmix64's published first output for state 0 + G
    assert int(truth.mix64(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF
