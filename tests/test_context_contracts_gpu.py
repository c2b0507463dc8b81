"""The argument contracts HipContext's wrappers share (raynet_amd/hip_implementations/context.py):
_table, _stack, _chk_mesh, _workspace, _chk_centers, the scene checker and the size entries, on the
smallest device tensors that reach each branch -- the exact minimum is taken and the right count
comes back; one element fewer, the wrong dtype, a strided view, a misaligned view, a host tensor
and (where the contract is not optional) None are refused with a ValueError that names the
argument.  No kernel is launched beyond what creating one small context needs."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(torch):
    from raynet_amd.hip_implementations.context import HipContext
    return HipContext(8, 4, 2, 4, 8, 8, 3, (0, 0, 0, 1, 1, 1), (4, 4, 4))


def _refused(call, name):
    with pytest.raises(ValueError, match=name):
        call()


def _misaligned(torch, shape, dtype):
    """A contiguous tensor of `shape` that starts one element into its buffer."""
    n = 1
    for s in shape:
        n *= s
    return torch.zeros((n + 1,), dtype=dtype, device="cuda")[1:].view(shape)


def test_table(torch):
    from raynet_amd.hip_implementations.context import _table
    f64, f32 = torch.float64, torch.float32
    cameras = torch.zeros((2, 15), dtype=f64, device="cuda")
    assert _table(cameras, 15, f64, "cameras", align=8) == 2
    assert _table(cameras, 15, f64, "cameras", align=8, rows=2) == 2
    assert _table(cameras[:0], 15, f64, "cameras", align=8) == 0
    wide = torch.zeros((2, 30), dtype=f64, device="cuda")
    for bad in (cameras[:, :14].contiguous(),               # one element fewer per row
                cameras.reshape(-1)[:29], cameras.reshape(-1), cameras.reshape(2, 15, 1),
                cameras.float(), wide[:, ::2], cameras.t().contiguous().t(), cameras.cpu(), None,
                cameras.cpu().numpy()):
        _refused(lambda: _table(bad, 15, f64, "cameras", align=8), "cameras")
    _refused(lambda: _table(cameras, 15, f64, "cameras", align=8, rows=3), r"cameras: expected a \(3, 15\)")
    _refused(lambda: _table(cameras, 15, f64, "cameras", align=8, rows=1), "cameras")
    # 16-byte rows: a view that starts one float into its buffer is refused, at 4 bytes taken
    xyzw = _misaligned(torch, (3, 4), f32)
    assert _table(xyzw, 4, f32, "ref_xyzw") == 3
    _refused(lambda: _table(xyzw, 4, f32, "ref_xyzw", align=16), "ref_xyzw.*16-byte")
    assert _table(torch.zeros((3, 4), dtype=f32, device="cuda"), 4, f32, "ref_xyzw", align=16) == 3


def test_stack(torch):
    from raynet_amd.hip_implementations.context import _stack
    images = torch.zeros((2, 3, 4, 1), dtype=torch.float32, device="cuda")
    maps = images[..., 0]
    assert _stack(images, 2, "images", channels=True) == (2, 3, 4, 1)
    assert _stack(images, None, "images", channels=True) == (2, 3, 4, 1)
    assert _stack(maps, 2, "depths") == (2, 3, 4) and _stack(maps, None, "depths") == (2, 3, 4)
    wide = torch.zeros((2, 3, 8, 1), dtype=torch.float32, device="cuda")
    for bad in (images[:1], maps, images.reshape(-1), images.double(), wide[:, :, ::2],
                images.cpu(), None):
        _refused(lambda: _stack(bad, 2, "images", channels=True), "images")
    for bad in (maps[:1], images, maps.reshape(-1)[:23], maps.half(), wide[:, :, ::2, 0],
                maps.cpu(), None):
        _refused(lambda: _stack(bad, 2, "depths"), "depths")


def test_mesh(torch):
    from raynet_amd.hip_implementations.context import _chk_mesh
    f32, i32 = torch.float32, torch.int32
    vertices = torch.zeros((3, 3), dtype=f32, device="cuda")
    faces = torch.zeros((1, 3), dtype=i32, device="cuda")
    offsets = torch.zeros((4,), dtype=i32, device="cuda")
    corners = torch.zeros((3,), dtype=i32, device="cuda")
    assert _chk_mesh(vertices, faces) == (3, 1)
    assert _chk_mesh(vertices, faces, offsets, corners) == (3, 1)
    assert _chk_mesh(vertices[:0], faces[:0], offsets[:1], corners[:0]) == (0, 0)
    wide = torch.zeros((3, 6), dtype=f32, device="cuda")
    for bad in (vertices.reshape(-1)[:8], vertices.double(), wide[:, ::2], vertices.cpu()):
        _refused(lambda: _chk_mesh(bad, faces, offsets, corners), "vertices")
    for bad in (faces.reshape(-1)[:2], faces.long(), faces.float(), faces.cpu()):
        _refused(lambda: _chk_mesh(vertices, bad), "faces")
    for bad in (offsets[:3], offsets.long(), torch.zeros((8,), dtype=i32, device="cuda")[::2],
                offsets.cpu(), None):
        _refused(lambda: _chk_mesh(vertices, faces, bad, corners), "offsets")
    for bad in (corners[:2], corners.short(), corners.cpu(), None):
        _refused(lambda: _chk_mesh(vertices, faces, offsets, bad), "corners")


def test_workspace(torch):
    from raynet_amd.hip_implementations.context import _workspace
    device = torch.device("cuda", torch.cuda.current_device())
    work = torch.zeros((48,), dtype=torch.uint8, device="cuda")
    assert _workspace(work[:24], 24, device).data_ptr() == work.data_ptr()
    assert _workspace(work, 24, device) is work
    for bad in (work[:23], work[:24].to(torch.int8), work[::2], work[1:25], work[4:28],
                work[:24].cpu()):
        _refused(lambda: _workspace(bad, 24, device), "workspace")
    for need, size in ((24, 24), (0, 8), (3, 8)):       # None: a fresh one, never empty
        fresh = _workspace(None, need, device)
        assert fresh.dtype == torch.uint8 and fresh.is_cuda and fresh.numel() == size
        assert fresh.data_ptr() % 8 == 0


def test_centers(torch):
    from raynet_amd.hip_implementations.context import _chk_centers
    c = torch.zeros((12,), dtype=torch.float32, device="cuda")
    assert _chk_centers(c[:3], 5, 0) is None            # one centre of three components
    _chk_centers(c, 5, 2)                               # ceil(5 / 2) groups of four
    _chk_centers(c[:4], 2, 2)
    _chk_centers(c[1:4], 5, 0)                          # (read element by element: 4 bytes)
    _chk_centers(None, 5, 2, optional=True)
    for bad, rpc in ((c[:2], 0), (c[:11], 2), (c.double(), 2), (c.cpu(), 0), (None, 0), (None, 2),
                     (torch.zeros((24,), dtype=torch.float32, device="cuda")[::2], 2)):
        _refused(lambda: _chk_centers(bad, 5, rpc), "center")


def test_host_arrays_texels_and_sizes(ctx):
    from raynet_amd.hip_implementations.context import _atlas_texels, _host3, _size
    d = _host3((3, 5.0, 7), ctypes.c_int32, "dims")
    assert isinstance(d, ctypes.c_int32 * 3) and list(d) == [3, 5, 7]
    o = _host3([0.5, -1, 2], ctypes.c_double, "origin")
    assert isinstance(o, ctypes.c_double * 3) and list(o) == [0.5, -1.0, 2.0]
    for bad in ((3, 5), (1.5, 2, 2), (3, 2 ** 31, 1), ((1, 2, 3),)):
        _refused(lambda: _host3(bad, ctypes.c_int32, "dims"), "dims")
    for bad in ((1.0, 2.0), 1.0, ((1.0, 2.0, 3.0),)):
        _refused(lambda: _host3(bad, ctypes.c_double, "cell"), "cell")
    # two faces share a cell of (T + 5)^2 texels, cells_per_row cells per row
    assert _atlas_texels(1, 1, 1) == 36 and _atlas_texels(2, 1, 1) == 36
    assert _atlas_texels(3, 1, 1) == 72 and _atlas_texels(7, 4, 3) == 3 * 9 * 2 * 9
    assert _atlas_texels(0, 4, 3) == 0
    for nf, T, cw in ((-1, 4, 3), (7, 0, 3), (7, 1025, 3), (7, 4, 0), (7, 4, 16385)):
        assert _atlas_texels(nf, T, cw) == 0
    assert _atlas_texels(7, 1024, 16384) == 16384 * 1029 * 1029
    assert _size(24, "rn_entry", nv=3) == 24 and _size(0, "rn_entry") == 0
    _refused(lambda: _size(-1, "rn_entry", nv=3, dims=(1, 2, 3)),
             r"rn_entry: bad sizes \(nv 3, dims \(1, 2, 3\)\)")
    # the size entries through it: the headers' arithmetic, and -1 as a ValueError
    assert ctx.mesh_fill_holes_workspace_bytes(0, 0) == 16 + 6144
    assert ctx.mesh_place_quadric_workspace_bytes(5, 0, 5) == 440
    assert ctx.mesh_simplify_workspace_bytes(0, 0, (3, 5, 7)) == 32 * 105
    assert ctx.mesh_smooth_workspace_bytes(3, 1) == 64      # ring 24 | scratch 36, to 8
    _refused(lambda: ctx.mesh_fill_holes_workspace_bytes(-1, 0), r"fill_holes.*nv -1, nf 0")
    _refused(lambda: ctx.mesh_place_quadric_workspace_bytes(5, 3, 6), r"quadric.*nv 5, nf 3, nvo 6")
    _refused(lambda: ctx.mesh_simplify_workspace_bytes(1, 1, (3, 0, 7)), r"simplify.*dims \(3, 0, 7\)")
    _refused(lambda: ctx.mesh_smooth_workspace_bytes(-1, 0), r"smooth.*nv -1, nf 0")


def test_scene_checker(torch, ctx):
    """What scene_prepare_all and scene_plan take alike (M = 8: rows are 16-byte aligned)."""
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    rows, n = 256, 5
    good = dict(ray_idxs=torch.zeros((n,), dtype=i32, device="cuda"),
                feature_table=torch.zeros((1, 2), dtype=i64, device="cuda"),
                cameras=torch.zeros((1, 40), dtype=f32, device="cuda"),
                vox=torch.zeros((rows * 8,), dtype=i32, device="cuda"),
                rvc=torch.zeros((rows,), dtype=i32, device="cuda"),
                Sr=torch.zeros((rows * 8,), dtype=f32, device="cuda"), order=None)
    assert ctx._chk_scene(1, rows, **good) == (n, rows)
    assert ctx._chk_scene(1, rows, **dict(good, order=good["ray_idxs"])) == (n, rows)
    for name, bad in (("ray_idxs", good["ray_idxs"].long()), ("ray_idxs", good["ray_idxs"].cpu()),
                      ("order", good["ray_idxs"][:4]), ("order", good["ray_idxs"].float()),
                      ("feature_table", good["feature_table"].int()),
                      ("cameras", good["cameras"].double()),
                      ("vox", good["vox"][:-1]), ("vox", _misaligned(torch, (rows * 8,), i32)),
                      ("vox", torch.zeros((rows * 16,), dtype=i32, device="cuda")[::2]),
                      ("rvc", good["rvc"][:-1]), ("rvc", None),
                      ("Sr", good["Sr"][:-1]), ("Sr", _misaligned(torch, (rows * 8,), f32))):
        _refused(lambda: ctx._chk_scene(1, rows, **dict(good, **{name: bad})), name)
    for name, bad in (("feature_table", good["feature_table"].reshape(-1)),
                      ("cameras", good["cameras"].reshape(-1))):
        with pytest.raises(AssertionError):
            ctx._chk_scene(1, rows, **dict(good, **{name: bad}))
    # a slice of the per-ray arrays is taken at any 4-byte offset
    six = torch.zeros((n + 1,), dtype=i32, device="cuda")
    assert ctx._chk_scene(1, rows, **dict(good, ray_idxs=six[1:], order=six[1:])) == (n, rows)
