"""The texture atlas on the GPU: rn_texture_bake and rn_texture_sample against
tests/texture_truth.py.  For every launch every output is PAD rows longer than asked and prefilled,
every input is compared bit for bit afterwards and the outputs EQUAL the truth's bits.  The shapes
are the smallest at which it can go wrong: one face (the upper half of its cell is empty), nine
faces three cells a row (odd, and a trailing empty cell), T = 1, T = 5 (cells of 10 texels: the
8 x 8 tiles straddle cells and the atlas's extents are no multiples of 8), 320 faces (several
workgroups); 1, 3 and 4 channels; 0, 1, 3 and 32 views (bit 31); with and without depth maps and
vertex normals; both modes; a zero-area face, faces that name no vertex, a NaN and an infinite
vertex, views behind the surface; the lookup on real rn_mesh_render planes with planted misses;
both entries' refusals; and the Python layers."""
import numpy as np
import pytest

import appearance_truth as at
import mesh_harness as h
import render_truth as rd
import texture_truth as tt

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
I = np.int32
FILL = -7.5
INVALID = -1
H, W = 12, 16


def _views(V, C, seed=0, with_depths=True):
    """V ring cameras around the origin at radius 3 -> (rows [V, 15] f64, images [V, H, W, C] f32,
    depths [V, H, W] f32 or None).  The depths belong to no surface: around the distance of the
    sphere's points to the cameras, so that the occlusion test passes for some texels and fails
    for others, with a zero, a negative, a NaN and an infinite value planted in every view."""
    from raynet_amd.synthetic import ring_cameras
    rng = np.random.default_rng(seed)
    # (the ring's default heights climb by 0.2 a view: 32 views would leave the depths' range)
    heights = None if V <= 3 else [0.3 + 0.01 * v for v in range(V)]
    cams = ring_cameras(V, H, W, focal=1.5 * H, heights=heights) if V else []
    rows = at.pack_cameras(cams).reshape(V, 15)
    images = rng.random((V, H, W, C)).astype(F)
    depths = None
    if with_depths:
        depths = rng.uniform(2.3, 3.0, size=(V, H, W)).astype(F)
        depths[:, 5, 7:11] = np.array([0, -1, np.nan, np.inf], F)
    return rows, images, depths


def _mesh(name):
    if name == "one":
        # (in the plane x = 0, its front towards the first camera of the ring)
        return np.array([[0, -0.5, -0.5], [0, 0.5, -0.5], [0, 0, 0.6]], F), np.array([[0, 1, 2]], I)
    if name == "nine":
        v, f = rd.icosphere(0)
        return v, f[:9]
    if name == "sphere":
        return rd.icosphere(2)
    assert name == "garbage"
    v, f = rd.icosphere(1)
    v, f = v.copy(), f.copy()
    f[3] = (f[3, 0], f[3, 0], f[3, 1])              # zero area: no facing test, weight 1
    f[5, 1] = len(v) + 7                            # names no vertex
    f[6, 0] = -1
    f[7] = (2 ** 31 - 1, -2 ** 31, 0)
    v[f[20, 0]] = np.nan
    v[f[40, 2], 1] = np.inf
    return v, f


def _bake(vertices, faces, L, rows, images, depths, normals, tol, min_cos, border, mode):
    """rn_texture_bake on device tensors, every output PAD texels longer than asked and prefilled
    -> (rc, the outputs as host arrays with their pads); the inputs are checked to be kept."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    V, Hh, Ww, C = images.shape
    n = L.Ht * L.Wt
    up = dict(vertices=(vertices, F), faces=(faces, I), normals=(normals, F), cameras=(rows, D),
              images=(images, F), depths=(depths, F))
    dev = {k: h.cuda(a, t) for k, (a, t) in up.items()}
    out = dict(texture=h.padded((n, C), FILL, torch.float32), weight=h.padded(n, FILL, torch.float32),
               views=h.padded(n, -77, torch.int32))
    rc = ctx.lib.rn_texture_bake(ctx._h, len(vertices), _ptr(dev["vertices"]), len(faces),
                                 _ptr(dev["faces"]), _ptr(dev["normals"]), L.T, L.Cw, V,
                                 _ptr(dev["cameras"]), Hh, Ww, C, _ptr(dev["images"]),
                                 _ptr(dev["depths"]), float(tol), float(min_cos), float(border),
                                 int(mode), _ptr(out["texture"]), _ptr(out["weight"]),
                                 _ptr(out["views"]), _stream())
    torch.cuda.synchronize()
    for k, (a, t) in up.items():
        if a is not None:
            h.assert_input_kept(dev[k], np.ascontiguousarray(a, t), k)
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _bake_is_the_truth(what, vertices, faces, T, Cw, V, C, with_depths=True, normals=None, tol=0.05,
                       min_cos=0.1, border=0.5, mode=0, seed=0):
    from raynet_amd import _lib
    L = tt.Layout(len(faces), T, Cw)
    rows, images, depths = _views(V, C, seed, with_depths)
    want = tt.bake(vertices, faces, L, rows, images, depths, normals, tol, min_cos, border, mode)
    rc, got = _bake(vertices, faces, L, rows, images, depths, normals, tol, min_cos, border, mode)
    assert rc == _lib.RN_OK, what
    n = L.Ht * L.Wt
    for k, fill in (("texture", FILL), ("weight", FILL), ("views", -77)):
        h.assert_untouched(got[k], n, fill, (what, k))
    seen = want[2] != 0
    print("%s: nf %d, T %d, %d x %d texels, V %d, C %d: %d owned, %d seen, masks %s" % (
        what, len(faces), T, L.Wt, L.Ht, V, C, int((tt.owners(L)[0] >= 0).sum()), int(seen.sum()),
        [hex(m) for m in np.unique(want[2])[:6]]))
    assert np.array_equal(got["views"][:n].view(np.uint32).reshape(L.Ht, L.Wt), want[2]), what
    h.assert_same_bits(got["weight"][:n].reshape(L.Ht, L.Wt), want[1], (what, "weight"))
    h.assert_same_bits(got["texture"][:n].reshape(L.Ht, L.Wt, C), want[0], (what, "texture"))
    return L, want


# ------------------------------------------------------------------------------ a. the bake
CASES = [
    # mesh, T, Cw, V, C, depths, vertex normals, mode
    ("one", 1, None, 1, 3, False, False, 0),
    ("one", 5, None, 3, 1, True, True, 1),
    ("nine", 1, 3, 3, 4, True, False, 0),
    ("nine", 5, 3, 3, 3, True, True, 0),
    ("nine", 5, 3, 0, 3, False, False, 0),
    ("nine", 4, 2, 1, 2, False, True, 1),
    ("sphere", 1, None, 3, 3, True, False, 1),
    ("sphere", 5, None, 3, 3, True, False, 0),
    ("sphere", 5, None, 3, 4, False, True, 1),
    ("sphere", 5, None, 32, 1, True, True, 0),
    ("sphere", 3, 40, 32, 3, False, False, 1),
    ("sphere", 2, 7, 0, 4, True, True, 0),
]


@pytest.mark.parametrize("name,T,Cw,V,C,with_depths,with_normals,mode", CASES)
def test_the_bake_is_the_truth(name, T, Cw, V, C, with_depths, with_normals, mode):
    vertices, faces = _mesh(name)
    normals = at.area_normals(vertices, faces) if with_normals else None
    L, want = _bake_is_the_truth(name, vertices, faces, T, Cw, V, C, with_depths, normals, mode=mode,
                                 seed=T + V)
    face = tt.owners(L)[0]
    assert (want[2][face < 0] == 0).all()
    if name == "one":
        assert (face < 0).sum() == L.S * L.S - (T + 4) * (T + 5) // 2      # the upper half
    if name == "nine" and Cw == 3:
        assert L.rows == 2 and (face[L.S:, 2 * L.S:] < 0).all()            # the trailing cell
    if V == 32:
        assert (want[2] >> 31).any(), "no texel sees view 31"
    if V and name == "sphere":
        assert (want[2] != 0).any()
    if V == 3 and name == "sphere":
        assert (want[2][face >= 0] == 0).any()


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_garbage_in_the_faces_and_the_vertices(with_normals, mode):
    vertices, faces = _mesh("garbage")
    normals = None
    if with_normals:
        normals = rd.vertex_attributes(len(vertices), 3, seed=4)[1]
        normals[5] = 0                  # a zero normal at a corner; and one that cancels inside
        normals[faces[30, 1]] = -normals[faces[30, 0]]
    L, want = _bake_is_the_truth("garbage", vertices, faces, 3, None, 3, 3, True, normals,
                                 tol=0.1, min_cos=0.0, border=0.0, mode=mode)
    face = tt.owners(L)[0]
    for f in (5, 6, 7, 20, 40):         # faces that name no vertex, or a vertex that is no point
        assert (want[2][face == f] == 0).all() and (want[0][face == f] == 0).all(), f
    if not with_normals:                # zero area: seen from both sides, every view weighs 1
        w = want[1][face == 3]
        assert (w == np.rint(w)).all()


def test_views_behind_the_surface_and_without_the_tests():
    """A camera ring around a closed surface: with the facing test every face is seen by some
    views only; without normals' help (min_cos 0, no depths, a zero-area mesh aside) the test is
    all that hides the back."""
    vertices, faces = _mesh("sphere")
    L, want = _bake_is_the_truth("behind", vertices, faces, 2, None, 3, 3, False, None, tol=0.0,
                                 min_cos=0.0, border=0.0, mode=0)
    face = tt.owners(L)[0]
    masks = want[2][face >= 0]
    assert (masks != 7).all() and (masks == 0).any() and (masks != 0).any()
    # the surface turned inside out is seen from behind only
    _, inside_out = _bake_is_the_truth("inside out", vertices, faces[:, ::-1].copy(), 2, None, 3, 3,
                                       False, None, tol=0.0, min_cos=0.0, border=0.0, mode=0)
    assert not np.array_equal(inside_out[2], want[2])


@pytest.mark.parametrize("mode", [0, 1])
def test_the_corner_texels_of_a_bake_are_rn_project_colors_at_the_vertices(mode):
    """texture_truth.corner_scene: at a chart's corner the texel's point and normal are the
    vertex's own, so both entries must give the same bits there -- the one test that would notice
    the two drifting apart (tests/test_texture_truth.py holds the truths to the same, and the
    scene to its conditions)."""
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    s = tt.corner_scene()
    V, Hh, Ww, C = s["images"].shape
    rc, baked = _bake(s["vertices"], s["faces"], s["L"], s["cameras"], s["images"], s["depths"],
                      s["normals"], s["tol"], s["min_cos"], s["border"], mode)
    assert rc == _lib.RN_OK
    n, Ht, Wt = s["L"].Ht * s["L"].Wt, s["L"].Ht, s["L"].Wt
    texel = tt.corners_of(s, (baked["texture"][:n].reshape(Ht, Wt, C),
                              baked["weight"][:n].reshape(Ht, Wt),
                              baked["views"][:n].view(np.uint32).reshape(Ht, Wt)))
    ctx = h.ctx()
    nv = len(s["vertices"])
    dev = [h.cuda(s[k], t) for k, t in (("vertices", F), ("normals", F), ("cameras", D),
                                        ("images", F), ("depths", F))]
    colors, weight = h.padded((nv, C), FILL, torch.float32), h.padded(nv, FILL, torch.float32)
    views = h.padded(nv, -77, torch.int32)
    ctx._check(ctx.lib.rn_project_colors(
        ctx._h, nv, _ptr(dev[0]), _ptr(dev[1]), V, _ptr(dev[2]), Hh, Ww, C, _ptr(dev[3]),
        _ptr(dev[4]), float(s["tol"]), float(s["min_cos"]), float(s["border"]), int(mode),
        _ptr(colors), _ptr(weight), _ptr(views), _stream()))
    order = s["faces"].reshape(-1)
    vertex = [colors.cpu().numpy()[:nv][order], weight.cpu().numpy()[:nv][order],
              views.cpu().numpy()[:nv].view(np.uint32)[order]]
    assert (vertex[2] != 0).all()
    assert np.array_equal(texel[2], vertex[2])
    h.assert_same_bits(texel[1], vertex[1], "weight")
    h.assert_same_bits(texel[0], vertex[0], "colours")
    # and both are the truth's
    want = at.project_colors(s["vertices"], s["normals"], s["cameras"], s["images"], s["depths"],
                             s["tol"], s["min_cos"], s["border"], mode)
    assert np.array_equal(vertex[2], want[2][order])
    h.assert_same_bits(vertex[0], want[0][order], "colours against the truth")


# ------------------------------------------------------------------------------ b. the lookup
def _sample(face, bary, L, texture, bilinear):
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    n, C = face.size, texture.shape[2]
    up = dict(face=(face, I), bary=(bary, F), texture=(texture, F))
    dev = {k: h.cuda(a, t) for k, (a, t) in up.items()}
    color = h.padded((n, C), FILL, torch.float32)
    rc = ctx.lib.rn_texture_sample(ctx._h, n, _ptr(dev["face"]), _ptr(dev["bary"]), L.nf, L.T, L.Cw,
                                   C, _ptr(dev["texture"]), int(bilinear), _ptr(color), _stream())
    torch.cuda.synchronize()
    for k, (a, t) in up.items():
        h.assert_input_kept(dev[k], np.ascontiguousarray(a, t), k)
    return rc, color.cpu().numpy()


@pytest.mark.parametrize("name,T,Cw,C", [("one", 1, None, 3), ("nine", 5, 3, 1), ("sphere", 5, None, 4),
                                         ("sphere", 1, 9, 3)])
def test_the_lookup_on_rendered_planes_is_the_truth(name, T, Cw, C):
    from raynet_amd import _lib
    from raynet_amd.mesh import MeshRaycaster
    vertices, faces = _mesh(name)
    rows = rd.ring_rows(2, 21, 27, focal=40.0)
    caster = MeshRaycaster(np.ascontiguousarray(vertices[faces], F).reshape(-1, 9))
    planes = caster._ctx.mesh_render(caster.nodes, caster.leaves, h.cuda(vertices, F),
                                     h.cuda(faces, I), h.cuda(rows, F), 21, 27)
    face, bary = planes[0].cpu().numpy().copy(), planes[2].cpu().numpy().copy()
    hits = np.argwhere(face >= 0)
    assert len(hits) > 8 and (face < 0).any()
    plant = [tuple(p) for p in hits[:: max(1, len(hits) // 8)][:8]]
    face[plant[0]] = len(faces)
    face[plant[1]] = 2 ** 31 - 1
    face[plant[2]] = -2 ** 31
    bary[plant[3]] = (np.nan, 0.25)
    bary[plant[4]] = (0.25, np.inf)
    bary[plant[5]] = (np.nextafter(F(1), F(2)), 0)
    bary[plant[6]] = (0, -np.nextafter(F(0), F(1)))
    bary[plant[7]] = (1, 1)             # each in range, their sum is not: still inside the cell
    L = tt.Layout(len(faces), T, Cw)
    texture = np.random.default_rng(T).random((L.Ht, L.Wt, C)).astype(F) + F(0.5)
    n = face.size
    for bilinear in (1, 0):
        want = tt.sample(face, bary, L, texture, bool(bilinear))
        rc, got = _sample(face, bary, L, texture, bilinear)
        assert rc == _lib.RN_OK
        h.assert_untouched(got, n, FILL, (name, "color"))
        h.assert_same_bits(got[:n].reshape(want.shape), want, (name, "bilinear %d" % bilinear))
        for p in plant[:7]:
            assert (want[p] == 0).all()
        assert (want[face < 0] == 0).all() and (want[plant[7]] != 0).all()
        print("%s: %d pixels, %d looked up, bilinear %d" % (name, n, int((want != 0).any(-1).sum()),
                                                            bilinear))


# ------------------------------------------------------------------------------ c. the refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    vertices, faces = _mesh("nine")
    rows, images, depths = _views(2, 3)
    L = tt.Layout(9, 2, 3)
    n = L.Ht * L.Wt
    dev = [h.cuda(a, t) for a, t in ((vertices, F), (faces, I), (rows, D), (images, F), (depths, F))]
    out = dict(texture=torch.full((n, 3), FILL, device="cuda"), weight=torch.full((n,), FILL, device="cuda"),
               views=torch.full((n,), -77, dtype=torch.int32, device="cuda"))
    null = _ptr(None)
    good = dict(nv=len(vertices), vertices=_ptr(dev[0]), nf=9, faces=_ptr(dev[1]), normals=null, T=2,
                Cw=3, V=2, cameras=_ptr(dev[2]), H=H, W=W, C=3, images=_ptr(dev[3]),
                depths=_ptr(dev[4]), tol=0.1, min_cos=0.0, border=0.0, mode=0,
                texture=_ptr(out["texture"]), weight=_ptr(out["weight"]), views=_ptr(out["views"]))

    def call(**change):
        a = dict(good)
        a.update(change)
        return ctx.lib.rn_texture_bake(ctx._h, *a.values(), _stream())

    def untouched():
        torch.cuda.synchronize()
        return bool((out["views"] == -77).all()) and all(
            (h.bits(out[k].cpu().numpy()) == h.bits(F(FILL))).all() for k in ("texture", "weight"))

    bad = [dict(nv=-1), dict(nf=-1), dict(nv=2 ** 31 - 1), dict(nf=(2 ** 31 - 1) // 3 + 1),
           dict(T=0), dict(T=-1), dict(T=1025), dict(Cw=0), dict(Cw=-3), dict(Cw=16385),
           dict(Cw=16384 // 7 + 1), dict(Cw=1, nf=2 * (16384 // 7) + 1),     # Wt, Ht > 16384
           dict(V=-1), dict(V=33), dict(C=0), dict(C=5), dict(H=0), dict(W=0), dict(H=-1),
           dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")), dict(min_cos=-0.1),
           dict(min_cos=1.0), dict(min_cos=float("nan")), dict(border=-1.0),
           dict(border=float("inf")), dict(mode=2), dict(mode=-1)]
    bad += [{name: null} for name in ("vertices", "faces", "texture", "weight", "views", "cameras",
                                      "images")]
    for change in bad:
        assert call(**change) == INVALID, change
        assert b"rn_texture_bake" in ctx.lib.rn_last_error(ctx._h), change
    assert ctx.lib.rn_texture_bake(None, *good.values(), _stream()) == INVALID
    assert untouched()
    # no face: RN_OK, nothing written, whatever the pointers
    nothing = {k: null for k in ("vertices", "faces", "cameras", "images", "texture", "weight", "views")}
    for change in (dict(nf=0), dict(nf=0, **nothing), dict(nf=0, nv=0, Cw=16384)):
        assert call(**change) == _lib.RN_OK, change
    assert untouched()
    # without views the cameras and the images are not read; normals and depths may be absent
    assert call(V=0, cameras=null, images=null, depths=null) == _lib.RN_OK
    torch.cuda.synchronize()
    assert bool((out["views"] == 0).all()) and bool((out["texture"] == 0).all())
    assert call() == _lib.RN_OK
    torch.cuda.synchronize()
    assert bool((out["views"] != 0).any())

    # ---- the lookup
    face = torch.zeros((10,), dtype=torch.int32, device="cuda")
    bary = torch.full((10, 2), 0.25, device="cuda")
    texture = torch.rand((L.Ht, L.Wt, 3), device="cuda") + 0.5
    color = torch.full((10, 3), FILL, device="cuda")
    good_s = dict(n=10, face=_ptr(face), bary=_ptr(bary), nf=9, T=2, Cw=3, C=3, texture=_ptr(texture),
                  bilinear=1, color=_ptr(color))

    def call_s(**change):
        a = dict(good_s)
        a.update(change)
        return ctx.lib.rn_texture_sample(ctx._h, *a.values(), _stream())

    bad = [dict(n=-1), dict(nf=-1), dict(nf=(2 ** 31 - 1) // 3 + 1), dict(T=0), dict(T=1025),
           dict(Cw=0), dict(Cw=16385), dict(C=0), dict(C=5), dict(bilinear=2), dict(bilinear=-1),
           dict(n=(2 ** 31 - 1) // 3 + 1), dict(Cw=16384 // 7 + 1), dict(Cw=1, nf=2 * (16384 // 7) + 1),
           dict(face=null), dict(bary=null), dict(color=null), dict(texture=null)]
    for change in bad:
        assert call_s(**change) == INVALID, change
        assert b"rn_texture_sample" in ctx.lib.rn_last_error(ctx._h), change
    assert ctx.lib.rn_texture_sample(None, *good_s.values(), _stream()) == INVALID
    torch.cuda.synchronize()
    assert (h.bits(color.cpu().numpy()) == h.bits(F(FILL))).all()
    for change in (dict(n=0), dict(n=0, face=null, bary=null, color=null, texture=null)):
        assert call_s(**change) == _lib.RN_OK
    torch.cuda.synchronize()
    assert (h.bits(color.cpu().numpy()) == h.bits(F(FILL))).all()
    # a mesh without faces: every pixel is a miss and the atlas is never read
    assert call_s(nf=0, texture=null) == _lib.RN_OK
    torch.cuda.synchronize()
    assert bool((color == 0).all())
    assert call_s() == _lib.RN_OK
    torch.cuda.synchronize()
    assert bool((color != 0).all())
    # the Python layers name the argument
    with pytest.raises(ValueError, match="texture"):
        ctx.texture_sample(face, bary, 9, 2, 3, texture[:-1].contiguous(), True, color)
    with pytest.raises(ValueError, match="views"):
        ctx.texture_bake(dev[0], dev[1], None, 2, 3, dev[2], dev[3], dev[4], 0.1, 0.0, 0.0, 0,
                         out["texture"], out["weight"], out["views"][:-1])


# ------------------------------------------------------------------------------ d. the package
def test_bake_texture_and_the_textured_render_are_the_truth(tmp_path):
    from PIL import Image as PILImage
    from raynet_amd import texture as tx
    from raynet_amd.synthetic import ring_cameras
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = rd.icosphere(1)
    mesh = SurfaceMesh(vertices, faces)
    cams = ring_cameras(3, H, W, focal=1.5 * H)
    rows, images, _ = _views(3, 3, seed=9, with_depths=False)
    caster = mesh.raycaster()
    maps = [caster.depth_map(cam, H, W) for cam in cams]
    depths = np.stack([np.asarray(m.cpu().numpy() if hasattr(m, "cpu") else m, F) for m in maps])
    L = tt.Layout(len(faces), 3)
    for normals, mode in (("face", "blend"), ("vertex", "best")):
        baked = tx.bake_texture(mesh, cams, list(images), 3, maps, tol=0.1, mode=mode, normals=normals)
        want = tt.bake(vertices, faces, L, rows, images, depths,
                       mesh.normals if normals == "vertex" else None, 0.1, 0.0, 0.0,
                       tx.MODES[mode])
        assert baked.layout == tx.atlas_layout(len(faces), 3)
        h.assert_same_bits(baked.texture.cpu().numpy(), want[0], (normals, "texture"))
        h.assert_same_bits(baked.weight.cpu().numpy(), want[1], (normals, "weight"))
        assert np.array_equal(baked.views.cpu().numpy().view(np.uint32), want[2])
    # the holes are filled where a face owns the texel, and only there
    owned, seen = tt.owners(L)[0] >= 0, want[2] != 0
    filled = baked.filled(unseen=(0.25, 0.5, 0.75))
    assert (owned & ~seen).any() and (filled[owned & ~seen] == np.array([0.25, 0.5, 0.75], F)).all()
    assert np.array_equal(filled[seen], want[0][seen]) and (filled[~owned] == 0).all()
    # the render looked up in the atlas
    render = mesh.render(cams, H, W, raycaster=caster)
    for bilinear in (True, False):
        got = render.textured(baked, bilinear)
        lookup = tt.sample(render.face.cpu().numpy(), render.bary.cpu().numpy(), L, want[0], bilinear)
        h.assert_same_bits(got.color.cpu().numpy(), lookup, ("textured", bilinear))
        assert got.face is render.face and got.rgb8(0).shape == (H, W, 3)
    # the file: the PNG's top row is row 0 of the atlas
    obj, mtl, png = mesh.save_obj(str(tmp_path / "ball.obj"), baked)
    assert np.array_equal(np.asarray(PILImage.open(png)), baked.rgb8())
    with pytest.raises(ValueError, match="32"):
        tx.bake_texture(mesh, ring_cameras(33, H, W), [images[0]] * 33, 3)
