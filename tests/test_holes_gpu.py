"""Hole filling on the GPU: rn_mesh_fill_holes against tests/holes_truth.py
-- all four outputs and the five counts EQUAL the truth's bits, the inputs are what they were, the
rows behind the counts and the bytes behind the workspace keep their prefill -- over the meshes of
tests/test_holes_truth.py (the smallest loop, tubes around the wavefront and the workgroup, the
punched sheet, the bow-tie, loops that stay open, garbage, the cut ball) and over a sheet of 180 k
faces whose half-edges outnumber one pass of the grid-stride loop and whose vertices need three
levels of the scan, a sheet with more filled loops than a scan tile holds, the same with its faces
permuted; the entry's refusals; and the chain from the depth maps of two spheres with a blanked
patch through the command line to a closed, smoothed mesh.  Every input is one the entry has to
survive by its guards."""
import os

import numpy as np
import pytest

import holes_truth as ht
import mesh_harness as h
import smooth_truth as st

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
I = np.int32
FILL = -7.5
INVALID = -1


def _launch(vertices, faces, offsets, corners, max_edges):
    """rn_mesh_fill_holes on device tensors, every output PAD rows longer than its bound and the
    workspace TAIL bytes longer than reported, all prefilled -> (rc, new_vertices, new_faces,
    source, counts, the four inputs on the device, the workspace, the bytes it needs)."""
    import torch
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    nv, nf = len(vertices), len(faces)
    v, f = h.cuda(np.reshape(vertices, (-1, 3)), F), h.cuda(np.reshape(faces, (-1, 3)), I)
    o, c = h.cuda(offsets, I), h.cuda(corners, I)
    need = int(ctx.lib.rn_mesh_fill_holes_workspace_bytes(nv, nf))
    assert need >= 32 * nv + 3 * nf + 16 and need % 8 == 0
    work = h.workspace(need)
    nvo = h.padded((nf, 3), FILL, torch.float32)
    nfo = h.padded((3 * nf, 3), -77, torch.int32)
    so = h.padded(nf, -77, torch.int32)
    counts = h.padded(5, -77, torch.int64)
    rc = ctx.lib.rn_mesh_fill_holes(ctx._h, nv, _ptr(v), nf, _ptr(f), _ptr(o), _ptr(c), int(max_edges),
                                    _ptr(nvo), _ptr(nfo), _ptr(so), _ptr(counts), _ptr(work),
                                    _stream())
    torch.cuda.synchronize()
    return (rc, nvo.cpu().numpy(), nfo.cpu().numpy(), so.cpu().numpy(), counts.cpu().numpy(),
            (v, f, o, c), work, need)


def _untouched(nvo, nfo, so, counts, work, need, k, m, what):
    """Nothing behind the k new vertices, the m new faces, the five counts and the workspace."""
    h.assert_untouched(counts, 5, -77, (what, "counts"))
    h.assert_untouched(nvo, k, FILL, (what, "new_vertices"))
    h.assert_untouched(nfo, m, -77, (what, "new_faces"))
    h.assert_untouched(so, k, -77, (what, "source"))
    h.assert_untouched(work, need, h.TAIL_BYTE, (what, "the workspace"))


def _same_as_truth(vertices, faces, max_edges, what, want=None):
    """All four outputs and the counts have the truth's bits, the inputs their own, the pads their
    prefill -> the truth's four arrays."""
    from raynet_amd import _lib
    vertices = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, I).reshape(-1, 3)
    offsets, corners = ht.corner_table(faces, len(vertices))
    if want is None:
        want = ht.fill(vertices, faces, max_edges)
    rc, nvo, nfo, so, counts, after, work, need = _launch(vertices, faces, offsets, corners,
                                                          max_edges)
    assert rc == _lib.RN_OK, what
    k, m = len(want[0]), len(want[1])
    print("%s: nv %d, nf %d, max_edges %d: counts %s (truth %s)"
          % (what, len(vertices), len(faces), max_edges, counts[:5].tolist(), want[3].tolist()))
    assert counts[:5].tolist() == want[3].tolist(), (what, counts[:5], want[3])
    _untouched(nvo, nfo, so, counts, work, need, k, m, what)
    for tensor, uploaded in zip(after, (vertices, faces, offsets, corners)):
        h.assert_input_kept(tensor, uploaded, what)
    h.assert_same_bits(nvo[:k], want[0], what)
    assert np.array_equal(nfo[:m], want[1]), what
    assert np.array_equal(so[:k], want[2]), what
    return want


# ------------------------------------------------------------------------------ a. the meshes
CASES = ht.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_every_mesh_of_the_truth(name):
    vertices, faces, max_edges = CASES[name]
    want = _same_as_truth(vertices, faces, max_edges, name)
    # the faces in another order: the truth's bits again, and the same loops, centres and faces
    again = _same_as_truth(vertices, ht.permuted(faces), max_edges, name + ", permuted")
    assert ht.same(again, want)


def test_the_properties_hold_on_the_gpus_result():
    from raynet_amd.smoothing import boundary_vertices
    vertices, faces = ht.tube(300)
    ctx = h.ctx()
    import torch
    from raynet_amd.appearance import corner_table
    v, f = torch.from_numpy(vertices).cuda(), torch.from_numpy(faces).cuda()
    new_vertices, new_faces, source, counts = ctx.mesh_fill_holes(v, f, *corner_table(f, len(v)), 300)
    assert counts.tolist() == [2, 600, 2, 0, 600] and source.tolist() == [0, 300]
    assert new_vertices.shape == (2, 3) and new_faces.shape == (600, 3)
    out_f = torch.cat([f, new_faces])
    assert ht.is_closed(out_f.cpu().numpy()) and not bool(boundary_vertices(out_f, len(v) + 2).any())
    # a second application adds nothing
    out_v = torch.cat([v, new_vertices])
    again = ctx.mesh_fill_holes(out_v, out_f, *corner_table(out_f, len(out_v)), 300)
    assert again[3].tolist() == [0, 0, 0, 0, 0] and len(again[0]) == 0 and len(again[1]) == 0


# ------------------------------------------------------------------------------ b. the sizes
@pytest.fixture(scope="module")
def large():
    """A 300 x 300 sheet with a 7 x 7 raster of punched cells: 90,601 vertices (three levels of
    the scan), 179,902 faces, 539,706 half-edges (more than 2048 x 256: the loop turns over)."""
    vertices, faces = ht.sheet(300, 300, [(40 * x + 20, 40 * y + 20) for x in range(7) for y in range(7)],
                               seed=11)
    assert len(vertices) == 301 * 301 and len(faces) == 2 * (300 * 300 - 49)
    assert 3 * len(faces) > 2048 * 256 and len(vertices) > 256 * 256
    return vertices, faces, ht.fill(vertices, faces, 16)


def test_a_sheet_larger_than_one_pass_of_the_grid(large):
    vertices, faces, want = large
    assert want[3].tolist() == [49, 196, 50, 0, 196 + 1200]
    _same_as_truth(vertices, faces, 16, "300 x 300 sheet", want)
    # with the rim: one walk of 1200 steps among 49 of 4
    _same_as_truth(vertices, faces, 1200, "300 x 300 sheet, rim too")
    _same_as_truth(vertices, faces, 1199, "300 x 300 sheet, rim one too long", want)


def test_more_filled_loops_than_a_scan_tile_holds_and_the_faces_permuted():
    vertices, faces = ht.raster_sheet(70, 2)
    want = _same_as_truth(vertices, faces, 16, "raster")
    assert want[3][0] == 34 * 34 > 256 and want[3][1] == 4 * 34 * 34 and want[3][2] == 34 * 34 + 1
    again = _same_as_truth(vertices, ht.permuted(faces, 3), 16, "raster, permuted")
    assert ht.same(again, want)


def test_three_launches_give_one_result(large):
    vertices, faces, want = large
    offsets, corners = ht.corner_table(faces, len(vertices))
    for _ in range(3):
        rc, nvo, nfo, so, counts = _launch(vertices, faces, offsets, corners, 16)[:5]
        assert rc == 0 and counts[:5].tolist() == want[3].tolist()
        assert np.array_equal(h.bits(nvo[:49]), h.bits(want[0])) and np.array_equal(nfo[:196], want[1])


def test_a_corner_table_that_is_not_the_meshs_reads_nothing_out_of_bounds():
    """Garbage in offsets and corners: the result is whatever the guarded gather gives, within the
    bounds of the outputs, and nothing beyond them is written."""
    from raynet_amd import _lib
    vertices, faces = ht.punched_sheet()
    offsets, corners = ht.corner_table(faces, len(vertices))
    rng = np.random.default_rng(13)
    junk = np.array([-1, 3 * len(faces), 2 ** 31 - 1, -2 ** 31, 0, 17], np.int64)
    off, cor = offsets.astype(np.int64), corners.astype(np.int64)
    hit = rng.random(len(off)) < 0.1
    off[hit] = rng.choice(junk, int(hit.sum()))
    hit = rng.random(len(cor)) < 0.1
    cor[hit] = rng.choice(junk, int(hit.sum()))
    rc, nvo, nfo, so, counts, _, work, need = _launch(vertices, faces, off.astype(I),
                                                      cor.astype(I), 10)
    assert rc == _lib.RN_OK
    k, m = int(counts[0]), int(counts[1])
    assert 0 <= k <= len(faces) and 0 <= m <= 3 * len(faces) and m <= counts[4] <= 3 * len(faces)
    _untouched(nvo, nfo, so, counts, work, need, k, m, "a table that is not the mesh's")
    assert ((nfo[:m] >= 0) & (nfo[:m] < len(vertices) + k)).all()


# ------------------------------------------------------------------------------ c. the refusals
def test_bad_arguments_are_refused_before_any_launch():
    import torch
    from raynet_amd import _lib
    from raynet_amd.hip_implementations.context import _ptr, _stream
    ctx = h.ctx()
    vertices, faces = ht.punched_sheet()
    nv, nf = len(vertices), len(faces)
    offsets, corners = ht.corner_table(faces, nv)
    v = torch.from_numpy(vertices).cuda()
    f = torch.from_numpy(faces).cuda()
    o = torch.from_numpy(offsets).cuda()
    c = torch.from_numpy(corners).cuda()
    need = int(ctx.lib.rn_mesh_fill_holes_workspace_bytes(nv, nf))
    work = torch.full((need + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    nvo = torch.full((nf, 3), FILL, dtype=torch.float32, device="cuda")
    nfo = torch.full((3 * nf, 3), -77, dtype=torch.int32, device="cuda")
    so = torch.full((nf,), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((5,), -77, dtype=torch.int64, device="cuda")
    null = _ptr(None)
    good = dict(nv=nv, vertices=_ptr(v), nf=nf, faces=_ptr(f), offsets=_ptr(o), corners=_ptr(c),
                max_edges=10, new_vertices=_ptr(nvo), new_faces=_ptr(nfo), source=_ptr(so),
                counts=_ptr(counts), workspace=_ptr(work))

    def call(**change):
        a = dict(good)
        a.update(change)
        return ctx.lib.rn_mesh_fill_holes(ctx._h, *a.values(), _stream())

    import ctypes
    odd = ctypes.c_void_p(work.data_ptr() + 4)
    bad = [dict(nv=-1), dict(nf=-1), dict(nv=2 ** 31 - 1), dict(nf=2 ** 31 // 3 + 1),
           dict(nv=2 ** 31 - 2 - nf + 1), dict(max_edges=2), dict(max_edges=0), dict(max_edges=-1),
           dict(max_edges=65537), dict(workspace=odd)]
    bad += [{name: null} for name in ("vertices", "faces", "offsets", "corners", "new_vertices",
                                      "new_faces", "source", "counts", "workspace")]
    bad += [dict(new_vertices=_ptr(v)), dict(new_faces=_ptr(f)), dict(source=_ptr(o)),
            dict(new_faces=_ptr(c)), dict(workspace=_ptr(nfo)), dict(source=_ptr(nvo)),
            dict(counts=_ptr(so)), dict(new_vertices=_ptr(work))]
    for change in bad:
        assert call(**change) == INVALID, change
        assert b"rn_mesh_fill_holes" in ctx.lib.rn_last_error(ctx._h), change
    assert ctx.lib.rn_mesh_fill_holes(None, *good.values(), _stream()) == INVALID
    torch.cuda.synchronize()
    assert (h.bits(nvo.cpu().numpy()) == h.bits(F(FILL))).all() and (nfo == -77).all()
    assert (so == -77).all() and (counts == -77).all() and (work == 0xA5).all()
    assert np.array_equal(h.bits(v.cpu().numpy()), h.bits(vertices)) and np.array_equal(f.cpu().numpy(), faces)
    assert ctx.lib.rn_mesh_fill_holes_workspace_bytes(-1, 0) == -1
    assert ctx.lib.rn_mesh_fill_holes_workspace_bytes(0, 2 ** 40) == -1
    assert ctx.lib.rn_mesh_fill_holes_workspace_bytes(2 ** 31 - 1, 0) == -1
    # nothing to do: the counts cleared, nothing else touched, whatever the other pointers
    for change in (dict(nv=0, nf=0), dict(nf=0), dict(nv=0),
                   dict(nf=0, faces=null, corners=null, new_vertices=null, new_faces=null,
                        source=null, workspace=null)):
        counts.fill_(-77)
        assert call(**change) == _lib.RN_OK, change
        torch.cuda.synchronize()
        assert counts.tolist() == [0] * 5, change
        assert (nfo == -77).all() and (so == -77).all() and (work == 0xA5).all(), change
    # the accepted edges of max_edges
    for ok in (3, 65536):
        assert call(max_edges=ok) == _lib.RN_OK
    # and the Python layers name the argument
    from raynet_amd.holes import fill_holes
    for kw, match in [(dict(max_edges=2), "max_edges"), (dict(max_edges=65537), "max_edges"),
                      (dict(faces=np.array([[0, 1, nv]])), "faces")]:
        args = dict(vertices=vertices, faces=faces, max_edges=10)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            fill_holes(**args)
    with pytest.raises(ValueError, match="workspace"):
        ctx.mesh_fill_holes(v, f, o, c, 10, workspace=work[:need - 8])


def test_fill_holes_and_surface_mesh_filled_are_the_truth():
    from raynet_amd.holes import fill_holes
    from raynet_amd.volume import SurfaceMesh
    vertices, faces = ht.punched_sheet()
    want = ht.filled_mesh(vertices, faces, 10)
    got = fill_holes(vertices, faces, 10)
    assert np.array_equal(h.bits(got[0]), h.bits(want[0])) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and got[3] == want[3]
    colors = np.random.default_rng(2).integers(0, 256, size=(len(vertices), 3)).astype(np.uint8)
    mesh = SurfaceMesh(vertices, faces, colors=colors)
    mesh.compute_normals()
    out = mesh.filled(10)
    assert np.array_equal(h.bits(out.vertices), h.bits(want[0])) and np.array_equal(out.faces, want[1])
    assert np.array_equal(out.colors[len(vertices):], colors[want[2]])
    assert out.normals.shape == out.vertices.shape and (out.normals[len(vertices):, 2] > 0).all()


# ------------------------------------------------------------------------------ d. the chain
def test_from_maps_with_a_blanked_patch_to_a_mesh_without_the_patchs_loops(tmp_path, capsys):
    from raynet_amd.scripts import fuse_depth_maps
    from raynet_amd.volume import SurfaceMesh
    bbox, cams, H, W, grid, big, small, gt_maps = h.two_sphere_maps(h.NOISE_SIGMA, h.NOISE_SEED,
                                                                    blank=h.PATCH)
    scene_dir, preds = str(tmp_path / "scene"), str(tmp_path / "predictions")
    h.write_restrepo_scene(scene_dir, bbox, cams, H, W, gt_maps)
    os.makedirs(preds)
    common = ["--gt", "--truncation", "0.25", "--start_end", "0,3", "--grid_shape", "18,22,14",
              "--keep_largest", "1", "--normals"]
    open_ply, closed_ply = str(tmp_path / "open.ply"), str(tmp_path / "closed.ply")
    assert fuse_depth_maps.main([scene_dir, preds, open_ply] + common) == 0
    assert "holes:" not in capsys.readouterr().out
    assert fuse_depth_maps.main([scene_dir, preds, closed_ply, "--fill_holes", "40", "--smooth", "5"]
                                + common) == 0
    printed = capsys.readouterr().out
    before, after = SurfaceMesh.load_ply(open_ply), SurfaceMesh.load_ply(closed_ply)
    # the truths applied in the chain's order to the unfilled file's mesh, to the bit
    vertices, faces, source, stats = ht.filled_mesh(before.vertices, before.faces, 40)
    side = float((2.0 / np.array(grid, D)).min())
    border = st.boundary_vertices(faces, len(vertices))
    want = st.smooth(vertices, faces, 5, 0.5, -0.53, border, side)
    assert np.array_equal(after.faces, faces)
    assert np.array_equal(h.bits(after.vertices), h.bits(want))
    # the printed line
    longer = stats["loops"] - stats["filled"] - stats["not_simple"]
    line = "holes: %d loops, %d filled (%d not simple, %d longer than 40), %d -> %d faces" % (
        stats["loops"], stats["filled"], stats["not_simple"], longer, len(before.faces), len(faces))
    assert line in printed.split("\n"), printed
    assert printed.index("components:") < printed.index("holes:") < printed.index("smooth:")
    # the patch's loops -- short and simple, where the ragged rim of the three views' caps is
    # neither -- are gone from the boundary; the rim is as it was
    assert stats["filled"] >= 2 and stats["loops"] > stats["filled"], stats
    _, a, b = ht.boundary_half_edges(before.faces, len(before.vertices))
    label = ht.loop_labels(a, b, len(before.vertices))
    on_filled = np.isin(label[a], source)
    was = st.boundary_vertices(before.faces, len(before.vertices))
    now = st.boundary_vertices(after.faces, len(after.vertices))
    assert was[a[on_filled]].all() and not now[a[on_filled]].any()
    assert np.array_equal(now[:len(was)][~np.isin(np.arange(len(was)), a[on_filled])],
                          was[~np.isin(np.arange(len(was)), a[on_filled])])
    assert not now[len(was):].any()
    print(line)
