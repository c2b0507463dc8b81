"""Rendering a mesh on the GPU: rn_mesh_render against tests/render_truth.py.
For every launch every output is PAD rows longer than asked and prefilled, every input is compared
bit for bit afterwards, the outputs EQUAL the truth's bits, and depth[v] has the bits
rn_mesh_depthmap writes for view v.  The meshes: one triangle, a coincident pair, a square seen
along its shared edge, an icosphere and the fused two-sphere mesh of the chain tests from three
cameras; images whose tiles hang over both edges and whose rows do not fill a wavefront; one pixel
more than a workgroup (the launch is not capped: there is no other path to reach); the faces
permuted; garbage in the faces, the vertices, the colours and the camera; the entry's refusals; and
the chain from coloured photographs through the command lines to a score."""
import json
import os

import numpy as np
import pytest

import mesh_harness as h
import raycast_truth as rt
import render_truth as rd

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
I = np.int32
FILL = -7.5
INVALID = -1


def _caster(triangles):
    from raynet_amd.mesh import MeshRaycaster
    return MeshRaycaster(np.ascontiguousarray(triangles, F).reshape(-1, 9))


def _launch(caster, vertices, faces, rows, H, W, colors=None, normals=None):
    """rn_mesh_render on device tensors, every output PAD rows (of pixels) longer than asked and
    prefilled -> (rc, dict of the outputs as host arrays with their pads, the inputs on the device
    and what was uploaded)."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    V, n = len(rows), len(rows) * H * W
    C = 0 if colors is None else colors.shape[1]
    up = dict(vertices=(vertices, F), faces=(faces, I), cameras=(rows, F), colors=(colors, F),
              normals=(normals, F))
    dev = {k: h.cuda(a, t) for k, (a, t) in up.items()}
    nodes_before, leaves_before = caster.nodes.cpu().numpy(), caster.leaves.cpu().numpy()
    out = dict(face=h.padded(n, -77, torch.int32), depth=h.padded(n, FILL, torch.float32),
               bary=h.padded((n, 2), FILL, torch.float32),
               color=None if colors is None else h.padded((n, C), FILL, torch.float32),
               normal=None if normals is None else h.padded((n, 3), FILL, torch.float32))
    rc = ctx.lib.rn_mesh_render(ctx._h, _ptr(caster.nodes), _ptr(caster.leaves), len(vertices),
                                _ptr(dev["vertices"]), len(faces), _ptr(dev["faces"]),
                                _ptr(dev["colors"]), C, _ptr(dev["normals"]), V, _ptr(dev["cameras"]),
                                H, W, _ptr(out["face"]), _ptr(out["depth"]), _ptr(out["bary"]),
                                _ptr(out["color"]), _ptr(out["normal"]), _stream())
    torch.cuda.synchronize()
    for k, (a, t) in up.items():
        if a is not None:
            h.assert_input_kept(dev[k], np.ascontiguousarray(a, t), k)
    h.assert_input_kept(caster.nodes, nodes_before, "nodes")
    h.assert_input_kept(caster.leaves, leaves_before, "leaves")
    return rc, {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _depthmaps(caster, rows, H, W):
    """rn_mesh_depthmap, one launch per view -> [V, H, W] f32."""
    import torch
    out = torch.empty((len(rows), H, W), dtype=torch.float32, device="cuda")
    for v, row in enumerate(np.ascontiguousarray(rows, F)):
        caster._ctx.mesh_depthmap(H, W, h.cuda(row[:12], F), h.cuda(row[12:], F), caster.nodes,
                                  caster.leaves, out[v])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_as_truth(vertices, faces, rows, H, W, colors=None, normals=None, what="", want=None,
                   triangles=None, caster=None):
    """One launch held to the truth and to rn_mesh_depthmap -> (the truth, the outputs)."""
    from raynet_amd import _lib
    vertices, faces = np.ascontiguousarray(vertices, F), np.ascontiguousarray(faces, I)
    rows = np.ascontiguousarray(rows, F).reshape(-1, 15)
    tri = vertices[faces].reshape(-1, 9) if triangles is None else triangles
    caster = _caster(tri) if caster is None else caster
    if want is None:
        want = rd.render(vertices, faces, rows, H, W, colors, normals, triangles=triangles)
    rc, got = _launch(caster, vertices, faces, rows, H, W, colors, normals)
    assert rc == _lib.RN_OK, what
    V, n = len(rows), len(rows) * H * W
    fills = dict(face=-77, depth=FILL, bary=FILL, color=FILL, normal=FILL)
    for k, a in got.items():
        assert (a is None) == (getattr(want, k) is None), (what, k)
        if a is not None:
            h.assert_untouched(a, n, fills[k], (what, k))
    hit = int((want.face >= 0).sum())
    print("%s: V %d, %d x %d, nf %d: %d of %d pixels hit" % (what, V, H, W, len(faces), hit, n))
    assert np.array_equal(got["face"][:n].reshape(V, H, W), want.face), what
    h.assert_same_bits(got["depth"][:n].reshape(V, H, W), want.depth, (what, "depth"))
    h.assert_same_bits(got["bary"][:n].reshape(V, H, W, 2), want.bary, (what, "bary"))
    if colors is not None:
        h.assert_same_bits(got["color"][:n].reshape(want.color.shape), want.color, (what, "color"),
                           nan_payloads=True)
    if normals is not None:
        h.assert_same_bits(got["normal"][:n].reshape(V, H, W, 3), want.normal, (what, "normal"))
    h.assert_same_bits(got["depth"][:n].reshape(V, H, W), _depthmaps(caster, rows, H, W),
                       (what, "rn_mesh_depthmap"))
    return want, got


# ------------------------------------------------------------------------------ a. by hand
def test_one_triangle_one_view():
    vertices, faces, corners = rd.one_triangle()
    colors = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]], F)
    normals = np.array([[0, 0, -1], [0.6, 0, -0.8], [0, 0.6, -0.8]], F)
    want, _ = _same_as_truth(vertices, faces, rd.axis_camera(8), 8, 8, colors, normals, "one triangle")
    assert (want.face[0] >= 0).sum() == 15 and all(want.face[0, y, x] == 0 for x, y in corners)


def test_of_a_coincident_pair_the_lower_face():
    vertices, faces = rd.coincident_pair()
    colors = np.repeat(np.array([[0.25], [0.75]], F), 3, axis=0)
    want, _ = _same_as_truth(vertices, faces, rd.axis_camera(8), 8, 8, colors, None, "coincident pair")
    assert want.ties.sum() == 15 and (want.face[want.face >= 0] == 0).all()


def test_rays_on_the_shared_edge_of_a_square():
    vertices, faces = rd.square()
    normals = np.array([[0, 0, -1]] * 4, F)
    want, _ = _same_as_truth(vertices, faces, rd.axis_camera(8), 8, 8, None, normals, "square")
    assert set(np.unique(want.face)) >= {-1, 0, 1}


# ------------------------------------------------------------------------------ b. the shapes
def test_three_views_of_seven_by_nine():
    """63 pixels per view: with a wavefront along the rows it would hold lanes of two views; with
    8 x 8 tiles, two tiles per view hang over both edges of the image."""
    vertices, faces = rd.icosphere(1)
    colors, normals = rd.vertex_attributes(len(vertices), 3, seed=1)
    want, _ = _same_as_truth(vertices, faces, rd.ring_rows(3, 7, 9), 7, 9, colors, normals, "7 x 9")
    assert all((want.face[v] >= 0).any() and (want.face[v] < 0).any() for v in range(3))


@pytest.mark.parametrize("V,H,W,focal", [(1, 3, 43, 60.0), (1, 1, 129, 200.0), (2, 17, 8, 25.0)])
def test_just_beyond_one_workgroup(V, H, W, focal):
    """129 pixels in rows (one more than a workgroup of 128), 17 tiles of one pixel's width in a
    row of tiles (one more than 16: eight workgroups and a half), 3 tiles per view over 2 views (a
    workgroup that holds the last tile of one view and the first of the next).  The launch is not
    capped: every workgroup is one more of the same, so there is no second size to reach."""
    vertices, faces = rd.icosphere(1)
    colors, normals = rd.vertex_attributes(len(vertices), 2, seed=2)
    want, _ = _same_as_truth(vertices, faces, rd.ring_rows(V, H, W, focal=focal), H, W, colors,
                             normals, "%d x %d x %d" % (V, H, W))
    assert (want.face >= 0).sum() > 20 and (want.face < 0).sum() > 20


# ------------------------------------------------------------------------------ c. real meshes
H3, W3 = 20, 30
_cache = {}


def _scene(name):
    """-> (vertices, faces, rows, colours of 4 channels, normals, the truth with both, the BVH),
    computed once per mesh: the channels are interpolated one by one, so the truth of fewer
    channels is the first ones of this."""
    if name not in _cache:
        if name == "icosphere":
            vertices, faces = rd.icosphere(2)
        else:
            from raynet_amd.fusion import fuse_depth_maps
            bbox, cams, H, W, grid, _, _, gt_maps = h.two_sphere_maps()
            assert (H, W) == (H3, W3)
            mesh = fuse_depth_maps(gt_maps, cams, bbox, grid, trunc=0.25).mesh()
            vertices, faces = mesh.vertices, mesh.faces
            assert 1000 < len(faces) < 20000
        rows = rd.ring_rows(3, H3, W3)
        colors, normals = rd.vertex_attributes(len(vertices), 4, seed=4)
        want = rd.render(vertices, faces, rows, H3, W3, colors, normals)
        _cache[name] = (vertices, faces, rows, colors, normals, want,
                        _caster(vertices[faces].reshape(-1, 9)))
    return _cache[name]


@pytest.mark.parametrize("C,with_normals", [(1, True), (3, True), (4, True), (3, False),
                                            (0, True), (0, False)])
@pytest.mark.parametrize("name", ["icosphere", "two spheres"])
def test_meshes_from_three_cameras(name, C, with_normals):
    vertices, faces, rows, colors, normals, full, caster = _scene(name)
    want = rd.Render()
    want.face, want.depth, want.bary, want.ties = full.face, full.depth, full.bary, full.ties
    want.color = np.ascontiguousarray(full.color[..., :C]) if C else None
    want.normal = full.normal if with_normals else None
    _same_as_truth(vertices, faces, rows, H3, W3,
                   np.ascontiguousarray(colors[:, :C]) if C else None,
                   normals if with_normals else None,
                   "%s, C %d%s" % (name, C, ", normals" if with_normals else ""), want=want,
                   caster=caster)
    assert (full.face >= 0).sum() > 150


def test_the_faces_permuted_give_the_same_images():
    vertices, faces, rows, colors, normals, full, _ = _scene("icosphere")
    # (equal keys go to the lower face, which a permutation changes: the truth finds none here)
    assert not full.ties.any()
    order = np.random.default_rng(5).permutation(len(faces))
    want, got = _same_as_truth(vertices, faces[order], rows, H3, W3, colors[:, :3].copy(), normals,
                               "icosphere, permuted")
    hit = full.face >= 0
    assert np.array_equal(want.face >= 0, hit) and np.array_equal(order[want.face[hit]], full.face[hit])
    for a, b in ((want.depth, full.depth), (want.bary, full.bary), (want.normal, full.normal),
                 (want.color, full.color[..., :3])):
        h.assert_same_bits(a, b, "permuted")


# ------------------------------------------------------------------------------ d. garbage
def test_garbage_in_faces_vertices_colours_and_camera():
    vertices, faces, rows, colors, normals, full, caster = _scene("icosphere")
    nv = len(vertices)
    colors = np.ascontiguousarray(colors[:, :3])
    # faces that name no vertex, among good ones; the BVH is the good faces' (a leaf's triangle
    # cannot be formed from such a face): face and depth stay, the rest is 0
    seen = np.unique(full.face[full.face >= 0])
    bad = faces.copy()
    bad[seen[0::4], 0] = -1
    bad[seen[1::4], 1] = nv
    bad[seen[2::4], 2] = 2 ** 31 - 1
    want, got = _same_as_truth(vertices, bad, rows, H3, W3, colors, normals, "faces that name no vertex",
                               triangles=vertices[faces].reshape(-1, 9), caster=caster)
    n = 3 * H3 * W3
    guarded = (full.face >= 0) & ~np.isin(full.face, seen[3::4])
    assert guarded.sum() > 100 and np.array_equal(want.face, full.face)
    for k in ("bary", "color", "normal"):
        a = got[k][:n].reshape(3, H3, W3, -1)
        assert (h.bits(a[guarded]) == 0).all(), k
    h.assert_same_bits(want.depth, full.depth, "guarded depth")
    # NaN vertices: their triangles are hit by nothing; NaN colours come through as NaN
    nan_vertices = vertices.copy()
    nan_vertices[faces[seen[0], 0]] = np.nan
    nan_vertices[faces[seen[5], 1], 1] = np.nan
    want, _ = _same_as_truth(nan_vertices, faces, rows, H3, W3, colors, normals, "NaN vertices")
    assert not np.isin(want.face, [seen[0], seen[5]]).any() and np.isfinite(want.color).all()
    nan_colors = colors.copy()
    nan_colors[faces[seen[1], 0], 1] = np.nan
    nan_colors[faces[seen[2], 2]] = np.inf
    want, _ = _same_as_truth(vertices, faces, rows, H3, W3, nan_colors, None, "NaN colours",
                             caster=caster)
    assert np.isnan(want.color).any() and np.isfinite(want.color[want.face < 0]).all()
    # a camera whose centre lies on the surface (on a vertex, inside a face), and one inside
    on = rows.copy()
    on[0, 12:] = vertices[faces[seen[0], 0]]
    on[1, 12:] = vertices[faces[seen[1]]].astype(D).mean(0).astype(F)
    on[2, 12:] = 0
    want, _ = _same_as_truth(vertices, faces, on, H3, W3, colors, normals, "centres on the surface",
                             caster=caster)
    assert (want.face[2] >= 0).mean() > 0.98       # (a ray through an edge may slip between two faces)


# ------------------------------------------------------------------------------ e. the refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    vertices, faces = rd.icosphere(0)
    rows = rd.ring_rows(2, 5, 6)
    caster = _caster(vertices[faces].reshape(-1, 9))
    colors, normals = rd.vertex_attributes(len(vertices), 3)
    dev = [h.cuda(a, t) for a, t in ((vertices, F), (faces, I), (colors, F), (normals, F), (rows, F))]
    n = 2 * 5 * 6
    out = dict(face=torch.full((n,), -77, dtype=torch.int32, device="cuda"),
               depth=torch.full((n,), FILL, device="cuda"), bary=torch.full((n, 2), FILL, device="cuda"),
               color=torch.full((n, 3), FILL, device="cuda"), normal=torch.full((n, 3), FILL, device="cuda"))
    null = _ptr(None)
    good = dict(nodes=_ptr(caster.nodes), leaves=_ptr(caster.leaves), nv=len(vertices),
                vertices=_ptr(dev[0]), nf=len(faces), faces=_ptr(dev[1]), colors=_ptr(dev[2]), C=3,
                normals=_ptr(dev[3]), V=2, cameras=_ptr(dev[4]), H=5, W=6, face=_ptr(out["face"]),
                depth=_ptr(out["depth"]), bary=_ptr(out["bary"]), color=_ptr(out["color"]),
                normal=_ptr(out["normal"]))

    def call(**change):
        a = dict(good)
        a.update(change)
        return ctx.lib.rn_mesh_render(ctx._h, *a.values(), _stream())

    def untouched():
        torch.cuda.synchronize()
        return (out["face"] == -77).all() and all(
            (h.bits(out[k].cpu().numpy()) == h.bits(F(FILL))).all() for k in ("depth", "bary", "color", "normal"))

    bad = [dict(nv=-1), dict(nf=-1), dict(V=-1), dict(H=-1), dict(W=-1), dict(V=4097),
           dict(nv=2 ** 31 - 1), dict(nf=(2 ** 31 - 1) // 3 + 1), dict(nf=0),
           dict(H=2 ** 16, W=2 ** 15, V=1), dict(V=2, H=2 ** 15, W=2 ** 15),
           dict(V=1, H=1, W=2 ** 31 - 1, C=2), dict(V=1, H=1, W=(2 ** 31 - 1) // 3 + 1),
           dict(C=0), dict(C=5), dict(C=-1),
           dict(color=null), dict(colors=null), dict(normal=null), dict(normals=null)]
    bad += [{name: null} for name in ("nodes", "leaves", "vertices", "faces", "cameras", "face",
                                      "depth", "bary")]
    for change in bad:
        assert call(**change) == INVALID, change
        assert b"rn_mesh_render" in ctx.lib.rn_last_error(ctx._h), change
    assert ctx.lib.rn_mesh_render(None, *good.values(), _stream()) == INVALID
    assert untouched()
    # nothing to do: RN_OK, nothing written, whatever the pointers
    nothing = {k: null for k in ("nodes", "leaves", "vertices", "faces", "cameras", "face", "depth",
                                 "bary", "colors", "color", "normals", "normal")}
    for change in (dict(V=0), dict(H=0), dict(W=0), dict(V=0, H=2 ** 31 - 1, W=2 ** 31 - 1),
                   dict(V=0, **nothing), dict(H=0, **nothing)):
        assert call(**change) == _lib.RN_OK, change
    assert untouched()
    # C is not read where there are no colours
    assert call(colors=null, color=null, C=99) == _lib.RN_OK
    # and the good call: all of it written
    assert call() == _lib.RN_OK
    torch.cuda.synchronize()
    assert not (h.bits(out["bary"].cpu().numpy()) == h.bits(F(FILL))).any()
    # the Python layers name the argument
    with pytest.raises(ValueError, match="cameras"):
        ctx.mesh_render(caster.nodes, caster.leaves, dev[0], dev[1], dev[4][:, :12].contiguous(), 5, 6)
    with pytest.raises(ValueError, match="colors"):
        ctx.mesh_render(caster.nodes, caster.leaves, dev[0], dev[1], dev[4], 5, 6,
                        colors=torch.zeros((len(vertices), 5), device="cuda"))
    with pytest.raises(ValueError, match="normals"):
        ctx.mesh_render(caster.nodes, caster.leaves, dev[0], dev[1], dev[4], 5, 6, normals=dev[3][:-1])
    with pytest.raises(ValueError, match="leaves"):
        ctx.mesh_render(caster.nodes, caster.leaves[:-1], dev[0], dev[1], dev[4], 5, 6)


def test_surface_mesh_render_is_the_truth_and_an_empty_mesh_raises():
    from raynet_amd.synthetic import ring_cameras
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = rd.icosphere(1)
    rng = np.random.default_rng(6)
    colors8 = rng.integers(0, 256, size=(len(vertices), 3)).astype(np.uint8)
    mesh = SurfaceMesh(vertices, faces, colors=colors8)
    mesh.compute_normals()
    cams = ring_cameras(2, 9, 11, focal=13.0)
    got = mesh.render(cams, 9, 11)
    want = rd.render(vertices, faces, rd.camera_rows(cams), 9, 11, colors8.astype(F) / F(255),
                     mesh.normals)
    assert np.array_equal(got.face.cpu().numpy(), want.face)
    assert np.array_equal(got.mask.cpu().numpy(), want.face >= 0)
    for k in ("depth", "bary", "color", "normal"):
        h.assert_same_bits(getattr(got, k).cpu().numpy(), getattr(want, k), k)
    # the images: 8-bit colours come back as they went in where a vertex fills the pixel's face
    rgb = got.rgb8(0, background=(1, 2, 3))
    assert rgb.shape == (9, 11, 3) and (rgb[want.face[0] < 0] == (1, 2, 3)).all()
    flat = SurfaceMesh(vertices, faces, colors=np.full((len(vertices), 3), 200, np.uint8))
    assert (flat.render(cams, 9, 11).rgb8(1)[want.face[1] >= 0] == 200).all()
    shaded = got.shaded8(0, cams)
    assert shaded.shape == (9, 11, 3) and (shaded[want.face[0] >= 0, 0] > 100).all()
    assert (shaded[want.face[0] < 0] == 0).all() and got.normal_rgb8(1).shape == (9, 11, 3)
    bare = SurfaceMesh(vertices, faces).render(cams, 9, 11, raycaster=mesh.raycaster())
    assert bare.color is None and bare.normal is None
    assert np.array_equal(bare.face.cpu().numpy(), want.face)
    with pytest.raises(ValueError, match="empty"):
        SurfaceMesh(vertices, np.zeros((0, 3), I)).render(cams, 9, 11)
    with pytest.raises(ValueError, match="raycaster"):
        SurfaceMesh(vertices, faces[:-1]).render(cams, 9, 11, raycaster=mesh.raycaster())


# ------------------------------------------------------------------------------ f. the chain
def _photograph(cam, H, W, maps):
    """(H, W, 3) uint8: the two spheres as the camera sees them, the colour a linear function of
    the 3-D point the pixel's ray hits (from the analytic depth), grey 51 where it hits nothing."""
    ys, xs = np.mgrid[0:H, 0:W]
    o, dst = rt.pixel_rays(cam.P_pinv, cam.center, xs.reshape(-1), ys.reshape(-1))
    ray = dst.astype(D) - o.astype(D)
    ray /= np.linalg.norm(ray, axis=1)[:, None]
    point = o.astype(D) + maps.reshape(-1, 1).astype(D) * ray
    colour = np.clip(0.5 + point * np.array([0.45, -0.45, 0.6]), 0, 1)
    colour[maps.reshape(-1) <= 0] = 0.2
    return np.rint(colour * 255).astype(np.uint8).reshape(H, W, 3)


def test_from_coloured_photographs_to_a_score(tmp_path, capsys):
    from PIL import Image as PILImage
    from raynet_amd.metrics import photometric_error
    from raynet_amd.scripts import fuse_depth_maps, render_mesh
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps()
    scene_dir, preds, out = str(tmp_path / "scene"), str(tmp_path / "predictions"), str(tmp_path / "out")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    photographs = [_photograph(cam, H, W, d) for cam, d in zip(cams, gt_maps)]
    for i, image in enumerate(photographs):
        PILImage.fromarray(image).save(os.path.join(scene_dir, "imgs", "frame_%03d.png" % i))
    os.makedirs(preds)
    ply = str(tmp_path / "mesh.ply")
    assert fuse_depth_maps.main([scene_dir, preds, ply, "--gt", "--truncation", "0.25", "--start_end",
                                 "0,3", "--grid_shape", "18,22,14", "--keep_largest", "1",
                                 "--color"]) == 0
    capsys.readouterr()
    assert render_mesh.main([scene_dir, ply, out, "--start_end", "0,3", "--compare", "--planes",
                             "color,normals,shaded,depth,faces", "--background", "51,51,51"]) == 0
    printed = capsys.readouterr().out.strip().split("\n")
    scores = json.load(open(os.path.join(out, "render_metrics.json")))["views"]
    assert len(printed) == 3 and len(scores) == 3
    for i in range(3):
        for pattern in ("render_%03d.png", "normals_%03d.png", "shaded_%03d.png", "depth_%03d.npy",
                        "faces_%03d.npy", "bary_%03d.npy"):
            assert os.path.isfile(os.path.join(out, pattern % i)), pattern % i
        s = scores[i]
        assert printed[i] == "view %d: coverage %.4f, mae %.4f, psnr %.2f" % (
            i, s["coverage"], s["mae"], s["psnr"])
        face = np.load(os.path.join(out, "faces_%03d.npy" % i))
        depth = np.load(os.path.join(out, "depth_%03d.npy" % i))
        assert face.shape == (H, W) and face.dtype == I and depth.dtype == F
        assert np.array_equal(depth > 0, face >= 0)
        assert 0 < s["coverage"] < 1 and s["coverage"] == (face >= 0).mean()
        render = np.asarray(PILImage.open(os.path.join(out, "render_%03d.png" % i)))
        assert (render[face < 0] == 51).all()
        # the coloured surface is closer to the photograph than the same surface painted in the
        # photograph's mean colour
        image = photographs[i].astype(F) / F(255)
        uniform = np.broadcast_to(image.reshape(-1, 3).mean(0), image.shape)
        flat = photometric_error(uniform, image, face >= 0)
        print("view %d: coverage %.4f, psnr %.2f dB coloured, %.2f dB in the mean colour"
              % (i, s["coverage"], s["psnr"], flat["psnr"]))
        assert s["psnr"] > flat["psnr"], (i, s, flat)
