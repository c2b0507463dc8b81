"""HipContext: one rn_ctx (include/raynet_hip.h) plus the torch plumbing.

The reference compiles one PyCUDA module per (M, D, N, F, H, W, padding, bbox,
grid_shape) tuple (cuda_implementations/raynet_fp.py:230-248); here the same
tuple creates one context and the kernels take the sizes at run time.  torch is
used for device memory and streams only.
"""
import ctypes

import numpy as np
import torch

from .. import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    """Raw device pointer of a tensor for the C ABI (NULL for None).  Every pointer handed to
    the library goes through here: it must be a contiguous CUDA tensor -- a strided view or a
    host tensor would be read as something else, silently."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("the C ABI takes contiguous CUDA tensors (got %s, %s)" % (
            "cuda" if t.is_cuda else "cpu", "contiguous" if t.is_contiguous() else "strided"))
    return ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype, min_numel=0, name="tensor", optional=False, align=4):
    """The C ABI takes raw device pointers: a tensor handed to it must be what the kernels
    assume -- on the GPU, contiguous, of the stated dtype, at least `min_numel` elements,
    `align`-byte aligned -- or the call fails HERE, not as a silent out-of-bounds access.
    Per-ray index / count arrays (ray_idxs, rvc, order, depth) are read element by element:
    4 bytes, so that any slice of them (a ray batch of 50, an odd shard bound) is accepted like
    the reference accepts it; the [n][M] row arrays are read with 128-bit accesses where M is a
    multiple of 4 (`HipContext._row_align`) and only then need 16."""
    if t is None:
        if optional:
            return t
        raise ValueError("%s: required" % name)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: expected a CUDA tensor" % name)
    if t.dtype != dtype:
        raise ValueError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s: must be contiguous" % name)
    if t.numel() < min_numel:
        raise ValueError("%s: %d elements, need >= %d" % (name, t.numel(), min_numel))
    if t.numel() and t.data_ptr() % align:
        raise ValueError("%s: data pointer is not %d-byte aligned" % (name, align))
    return t


def _chk_mesh(vertices, faces, *table):
    """A mesh as the mesh entries take it: vertices (nv, 3) f32, faces (nf, 3) i32 and, where the
    entry reads one, the corner table (offsets [nv + 1] i32, corners [3 nf] i32) -> (nv, nf)."""
    nv, nf = len(vertices), len(faces)
    _chk(vertices, torch.float32, 3 * nv, "vertices")
    _chk(faces, torch.int32, 3 * nf, "faces")
    if table:
        offsets, corners = table
        _chk(offsets, torch.int32, nv + 1, "offsets")
        _chk(corners, torch.int32, 3 * nf, "corners")
    return nv, nf


def _workspace(workspace, need, device):
    """The uint8 workspace of an entry that reports `need` bytes: the given one, at least that
    long and 8-byte aligned, or a fresh one (never empty: the entry wants a pointer)."""
    if workspace is None:
        return torch.empty((max(need, 8),), dtype=torch.uint8, device=device)
    return _chk(workspace, torch.uint8, need, "workspace", align=8)


def _table(t, k, dtype, name, align=4, rows=None):
    """A table as the entries take one: a 2-D tensor of `k` columns (and, if given, exactly `rows`
    rows) that passes _chk -> its row count."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != k or \
            rows is not None and t.shape[0] != rows:
        raise ValueError("%s: expected a (%s, %d) tensor, got %s" % (
            name, "n" if rows is None else rows, k,
            tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    n = int(t.shape[0])
    _chk(t, dtype, k * n, name, align=align)
    return n


def _stack(t, V, name, channels=False):
    """A stack of float32 maps (V, H, W) or, with channels, of images (V, H, W, C), V given or
    (None) the stack's own -> its shape."""
    dims = 4 if channels else 3
    if not isinstance(t, torch.Tensor) or t.dim() != dims or V is not None and t.shape[0] != V:
        raise ValueError("%s: expected (%s, H, W%s), got %s" % (
            name, "V" if V is None else V, ", C" if channels else "",
            tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    _chk(t, torch.float32, t.numel(), name)
    return tuple(int(s) for s in t.shape)


def _atlas_texels(n_faces, T, cells_per_row):
    """Texels of the atlas of n_faces faces, T steps per leg, cells_per_row cells per row (two
    faces share a cell of (T + 5)^2); 0 for the sizes the entries refuse themselves."""
    if not (1 <= T <= 1024 and 1 <= cells_per_row <= 16384 and n_faces >= 0):
        return 0
    cell_rows = ((n_faces + 1) // 2 + cells_per_row - 1) // cells_per_row
    return cells_per_row * (T + 5) * cell_rows * (T + 5)


def _host3(x, ctype, name):
    """Three host numbers as the array an entry takes for `const T name[3]`: whole int32 numbers
    for c_int32, any numbers for c_double."""
    if ctype is ctypes.c_int32:
        a = np.asarray(x)
        if a.shape != (3,) or not np.all(a == np.floor(a)) or np.any(np.abs(a) >= 2 ** 31):
            raise ValueError("%s: three whole numbers, got %r" % (name, x))
        return (ctype * 3)(*[int(v) for v in a])
    a = np.asarray(x, np.float64)
    if a.shape != (3,):
        raise ValueError("%s: three numbers, got %r" % (name, x))
    return (ctype * 3)(*[float(v) for v in a])


def _size(answer, entry, **sizes):
    """A size entry's answer, or a ValueError naming its arguments (the entries answer -1)."""
    if answer < 0:
        raise ValueError("%s: bad sizes (%s)" % (entry, ", ".join("%s %s" % s for s in sizes.items())))
    return int(answer)


def _chk_centers(center, n, rays_per_center, optional=False):
    """The centres of the depth sweeps: one [3] for all n rays or, with rays_per_center > 0, a
    table [groups][4] of one per group of that many rays."""
    need = 4 * ((n + rays_per_center - 1) // rays_per_center) if rays_per_center > 0 else 3
    _chk(center, torch.float32, need, "center", optional=optional, align=4)


SCATTER_ITEM_TILES = 1 << 19      # tiles an int32 item `tile << 12 | ...` can name


def scatter_work_list(rvc, M, level=0, target_items=2048):
    """int32 items `tile << 12 | first chunk << 6 | chunks` for the LDS-box scatter at tile
    `level` (0: 128 rays x 32 steps, 1: 256 x 16) from the rays' voxel counts [rows]: a tile's
    LIVE chunks (up to its longest sending ray; rays with <= 1 voxels send nothing, mrf_np.py:300)
    in items of U chunks, U such that the launch has about `target_items` workgroups -- a tile of
    long rays becomes several items, a border tile one, a tile no ray of which sends anything none
    -- sorted longest first, tiles in order within a length.  None when nothing is live."""
    tile, steps = (128, 32) if level == 0 else (256, 16)
    c = rvc.to(torch.int64).clamp(max=M)
    c = torch.where(c <= 1, torch.zeros_like(c), c)
    pad = (-c.numel()) % tile
    if pad:
        c = torch.cat([c, torch.zeros((pad,), dtype=c.dtype, device=c.device)])
    nch = (c.view(-1, tile).max(1).values + steps - 1) // steps          # live chunks per tile
    total = int(nch.sum().item())
    if total == 0 or len(nch) > SCATTER_ITEM_TILES:
        # (an item's tile field has 19 bits: a larger plan keeps the scatter's tiles x split launch;
        # rn_scene_bind_scatter_items refuses such rows as well)
        return None
    U = int(min(63, max(1, -(-total // int(target_items)))))
    per_tile = (nch + U - 1) // U                                        # items per tile
    tile_of = torch.repeat_interleave(torch.arange(len(nch), device=c.device), per_tile)
    first = torch.cumsum(per_tile, 0) - per_tile
    begin = (torch.arange(len(tile_of), device=c.device) - first[tile_of]) * U
    cnt = torch.minimum(torch.full_like(begin, U), nch[tile_of] - begin)
    order = torch.sort(-cnt, stable=True).indices
    return ((tile_of << 12) | (begin << 6) | cnt)[order].to(torch.int32).contiguous()


def to_device(x, dtype=None, device="cuda"):
    """The reference's `to_gpu` / all_arrays_to_gpu (cuda_implementations/utils.py:11-22):
    NumPy arrays are uploaded, device tensors pass through untouched."""
    if isinstance(x, torch.Tensor):
        t = x
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        if not t.is_cuda:
            t = t.to(device)
        return t.contiguous()
    a = np.ascontiguousarray(x)
    t = torch.from_numpy(a)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.to(device)


class HipContext(object):
    def __init__(self, M, D, N, F, H, W, padding, bbox, grid_shape, device=None):
        if not torch.cuda.is_available():
            raise _lib.RaynetHipError(
                "no GPU visible: raynet_amd runs its hot path on MI355X only (no CPU fallback)")
        self.lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else device)
        bbox = np.asarray(bbox, dtype=np.float32).reshape(-1)
        assert bbox.shape == (6,)
        grid_shape = [int(g) for g in np.asarray(grid_shape).reshape(-1)]
        assert len(grid_shape) == 3
        cfg = _lib.Config()
        cfg.M, cfg.D, cfg.N, cfg.F = int(M), int(D), int(N), int(F)
        cfg.H, cfg.W, cfg.padding = int(H), int(W), int(padding)
        for i in range(3):
            cfg.grid[i] = grid_shape[i]
        for i in range(6):
            cfg.bbox[i] = float(bbox[i])
        cfg.device = self.device.index
        self.M, self.D, self.N, self.F = int(M), int(D), int(N), int(F)
        self.H, self.W, self.padding = int(H), int(W), int(padding)
        self.bbox = bbox
        self.grid_shape = tuple(grid_shape)
        self.G = grid_shape[0] * grid_shape[1] * grid_shape[2]
        self.feature_shape = (self.N, self.H + self.padding + 1, self.W + self.padding + 1, self.F)
        # rows of the [n][M] arrays start 16-byte aligned iff M % 4 == 0 -- exactly when the
        # kernels use their 128-bit row accesses (k_traverse's flush, k_scatter_slab's loads)
        self._row_align = 16 if self.M % 4 == 0 else 4
        handle = ctypes.c_void_p()
        rc = self.lib.rn_create(ctypes.byref(cfg), ctypes.byref(handle))
        if rc != _lib.RN_OK:
            raise _lib.RaynetHipError("rn_create failed: %s" % _lib.STATUS.get(rc, rc))
        self._h = handle
        self._options = None            # the rn_options last applied (set_options)
        # what the context keeps alive, or knows about the bindings the library holds pointers of
        self._grid_set = False
        self._vg_keepalive = None       # the voxel centres rn_set_voxel_grid was given
        self._grid_src = None           # the caller's array they were made from (the K-API drivers)
        self._slab_boxes = None         # (table, vox) of bind_slab_boxes
        self._scatter_items = None      # (items, vox, level) of bind_scatter_items
        self._seg_scratch = None        # [rows][8] f32 the traversal leaves the rays' segments in
        # profiling (prof_begin / prof_end)
        self._prof_cap = 0
        self.prof_active = False        # event pairs around launches: such a pass is not captured
        self.prof_starts = []

    def set_options(self, options):
        """Apply a PathOptions' context half (rn_options); a no-op when nothing changed."""
        want = options.context_options()
        if self._options == want:
            return
        o = _lib.Options(*want)
        self._check(self.lib.rn_set_options(self._h, ctypes.byref(o)))
        self._options = want

    def get_options(self):
        o = _lib.Options()
        self._check(self.lib.rn_get_options(self._h, ctypes.byref(o)))
        return dict(scatter_mode=o.scatter_mode, box_level=o.box_level, box_pin=bool(o.box_pin),
                    overlap=o.overlap, generic_sweep=bool(o.generic_sweep),
                    sweep_rays_per_wave=o.sweep_rays_per_wave)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.lib.rn_destroy(h)
            self._h = None

    # ------------------------------------------------------------------
    def _check(self, rc):
        if rc != _lib.RN_OK:
            raise _lib.RaynetHipError("%s: %s" % (
                _lib.STATUS.get(rc, rc), self.lib.rn_last_error(self._h).decode()))

    def dev(self, x, dtype=None):
        return to_device(x, dtype, self.device)

    def set_voxel_grid(self, voxel_grid):
        vg = self.dev(voxel_grid, torch.float32)
        assert vg.numel() == self.G * 3
        self._check(self.lib.rn_set_voxel_grid(self._h, _ptr(vg), _stream()))
        self._grid_set = True
        self._vg_keepalive = vg

    def acc_copies(self):
        return int(self.lib.rn_acc_copies(self._h))

    def scatter_reset(self):
        self._check(self.lib.rn_scatter_reset(self._h))

    def bind_slab_boxes(self, vox, table=None):
        """Let rn_scene_prepare_all keep slab boxes for the list buffer `vox` ([rows][M] i32;
        None unbinds): the scatters of a pass then merge boxes instead of scanning the lists
        (include/raynet_hip.h).  Returns the scratch table (pass it back in to re-bind the same
        buffer later: contexts are shared, the binding is the last caller's)."""
        if vox is None:
            self._check(self.lib.rn_scene_bind_slab_boxes(self._h, None, 0, None))
            self._slab_boxes = None
            return None
        _chk(vox, torch.int32, self.M, "vox", align=self._row_align)
        rows = vox.numel() // self.M
        size = int(self.lib.rn_slab_boxes_size(self._h, rows))
        if table is None:
            table = torch.empty((size,), dtype=torch.int32, device=self.device)
        _chk(table, torch.int32, size, "slab-box table", align=8)
        self._slab_boxes = (table, vox)
        self._check(self.lib.rn_scene_bind_slab_boxes(self._h, _ptr(vox), rows, _ptr(table)))
        return table

    def bind_scatter_items(self, vox, rvc=None, level=0, target_items=2048, items=None):
        """Work list of the LDS-box scatter over ALL rows of `vox` ([rows][M]; None unbinds), built
        from the rays' voxel counts `rvc` [rows] by scatter_work_list (or `items`: a list built
        before, to bind again -- contexts are shared, the binding is the last caller's).  One host
        synchronisation (the item count) per build; the list depends on the counts only, i.e. on
        cameras and shard, not on a pass (rn_scene_bind_scatter_items)."""
        if vox is None:
            self._check(self.lib.rn_scene_bind_scatter_items(self._h, None, 0, 0, None, 0))
            self._scatter_items = None
            return None
        rows = vox.numel() // self.M
        if items is None:
            items = scatter_work_list(rvc, self.M, level, target_items)
        if items is None or items.numel() == 0:
            return self.bind_scatter_items(None)
        _chk(items, torch.int32, 1, "scatter items")
        self._scatter_items = (items, vox, level)
        self._check(self.lib.rn_scene_bind_scatter_items(self._h, _ptr(vox), rows, int(level),
                                                         _ptr(items), int(items.numel())))
        return items

    def scatter_items_bound(self, items):
        cur = self._scatter_items
        return cur is not None and cur[0] is items

    def slab_boxes_bound_to(self, vox):
        sb = self._slab_boxes
        return sb is not None and sb[1] is vox

    def scatter_state(self):
        """-> (tile level in use, chunks, overflowed chunks of the last counted launch)"""
        lv, ch, ov = ctypes.c_int32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.rn_scatter_state(self._h, ctypes.byref(lv), ctypes.byref(ch),
                                              ctypes.byref(ov)))
        return int(lv.value), int(ch.value), int(ov.value)

    def scatter_settled(self):
        """No scatter launch touches the host any more and the tile shape stays as it is
        (rn_scatter_settled): a step's launches may be recorded into a HIP graph."""
        return bool(self.lib.rn_scatter_settled(self._h))

    # resident accumulators are 4x4x4-bricked (include/raynet_hip.h); the reference's
    # [gx][gy][gz] view is produced / consumed through these two
    def acc_size(self):
        return int(self.lib.rn_acc_size(self._h))

    def acc_to_grid(self, acc):
        out = torch.empty(self.grid_shape, dtype=torch.float32, device=acc.device)
        self._check(self.lib.rn_acc_to_grid(self._h, _ptr(acc), _ptr(out), _stream()))
        return out

    def stitch_rows(self, rows, index, out):
        """out[i] = rows[index[i]] (rn_stitch_rows) on the current stream; `out` is a CUDA tensor
        or a PINNED host tensor -- the kernel then writes the map across PCIe itself.  The
        caller vouches for index < rows.numel() (a plan checks its tables once)."""
        n = int(index.numel())
        _chk(rows, torch.float32, 1 if n else 0, "rows")
        _chk(index, torch.int32, n, "index", align=16)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and
                out.is_contiguous() and out.numel() >= n and (out.is_cuda or out.is_pinned()) and
                (n == 0 or out.data_ptr() % 16 == 0)):
            raise ValueError("out: expected a contiguous float32 CUDA or pinned tensor of >= %d "
                             "elements, 16-byte aligned" % n)
        self._check(self.lib.rn_stitch_rows(self._h, n, _ptr(rows), _ptr(index), out.data_ptr(),
                                            _stream()))
        return out

    def acc_from_grid(self, grid):
        grid = self.dev(grid, torch.float32).contiguous()
        out = torch.zeros((self.acc_size(),), dtype=torch.float32, device=grid.device)
        self._check(self.lib.rn_acc_from_grid(self._h, _ptr(grid), _ptr(out), _stream()))
        return out

    # ---- the occupancy volume (raynet_amd/volume.py) --------------------------------------
    def occupancy_grid(self, acc, bricked, bias=0.0, out=None):
        """rn_occupancy_grid: -> belief [gx][gy][gz] f32 = occupancy_to_ray(bias + acc, 0) per
        voxel.  acc: the bricked buffer of acc_size() floats (bricked=True) or the [gx][gy][gz]
        array (bricked=False)."""
        _chk(acc, torch.float32, self.acc_size() if bricked else self.G, "accumulator")
        if out is None:
            out = torch.empty(self.grid_shape, dtype=torch.float32, device=acc.device)
        _chk(out, torch.float32, self.G, "belief")
        self._check(self.lib.rn_occupancy_grid(self._h, _ptr(acc), 1 if bricked else 0,
                                               float(bias), _ptr(out), _stream()))
        return out

    def volume_render(self, starts, ends, center, belief, out):
        """rn_volume_render: starts / ends (n, 3), center [3], belief [gx][gy][gz] -> out
        (5, S >= n) f32: depth, opacity, expected depth, confidence, median depth; ray i at
        out[:, i], nothing written at out[:, n:]."""
        n = len(starts)
        _chk(starts, torch.float32, 3 * n, "starts")
        _chk(ends, torch.float32, 3 * n, "ends")
        _chk(center, torch.float32, 3, "center")
        _chk(belief, torch.float32, self.G, "belief")
        _chk(out, torch.float32, 5 * n, "out")
        if len(ends) != n or out.dim() != 2 or out.shape[0] != 5 or out.shape[1] < n:
            raise ValueError("ends (%d, 3) and out (5, >= %d): got %s, %s"
                             % (n, n, tuple(ends.shape), tuple(out.shape)))
        self._check(self.lib.rn_volume_render(self._h, n, _ptr(starts), _ptr(ends), _ptr(center),
                                              _ptr(belief), _ptr(out), int(out.shape[1]),
                                              _stream()))
        return out

    def isosurface(self, belief, iso, closed=True):
        """rn_isosurface_count / rn_isosurface_emit: the iso-surface of belief [gx][gy][gz] f32 at
        `iso` by marching tetrahedra -> (vertices (nv, 3) f32, faces (nf, 3) int32), device
        tensors in the definition's order (include/raynet_hip.h).  closed: the grid is padded
        with one layer of zeros, so the surface is closed.  Synchronises the stream once (the
        totals come back to the host to size the outputs)."""
        _chk(belief, torch.float32, self.G, "belief")
        closed = 1 if closed else 0
        size = int(self.lib.rn_isosurface_workspace_bytes(self._h, closed))
        if size < 0:
            raise ValueError("isosurface: the lattice of a %s grid is too large" % (self.grid_shape,))
        work = torch.empty((size,), dtype=torch.uint8, device=belief.device)
        totals = (ctypes.c_int64 * 2)()
        self._check(self.lib.rn_isosurface_count(self._h, _ptr(belief), float(iso), closed,
                                                 _ptr(work), totals, _stream()))
        nv, nf = int(totals[0]), int(totals[1])
        vertices = torch.empty((nv, 3), dtype=torch.float32, device=belief.device)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=belief.device)
        self._check(self.lib.rn_isosurface_emit(self._h, _ptr(belief), float(iso), closed,
                                                _ptr(work), nv, nf, _ptr(vertices), _ptr(faces),
                                                _stream()))
        return vertices, faces

    # ---- normals and colours (raynet_amd/appearance.py) --------------------------------------
    def vertex_area_normals(self, vertices, faces, offsets, corners, normals=None):
        """rn_vertex_area_normals: vertices (nv, 3) f32, faces (nf, 3) i32 and the mesh's corner
        table by vertex (offsets [nv + 1] i32, corners [3 nf] i32) -> normals (nv, 3) f32, the
        area-weighted sums of the face normals around every vertex (not normalised)."""
        nv, nf = _chk_mesh(vertices, faces, offsets, corners)
        if normals is None:
            normals = torch.empty((nv, 3), dtype=torch.float32, device=vertices.device)
        _chk(normals, torch.float32, 3 * nv, "normals")
        self._check(self.lib.rn_vertex_area_normals(self._h, nv, _ptr(vertices), nf, _ptr(faces),
                                                    _ptr(offsets), _ptr(corners), _ptr(normals),
                                                    _stream()))
        return normals

    def project_colors(self, points, normals, cameras, images, depths, tol, min_cos, border, mode,
                       colors, weight, views):
        """rn_project_colors: points (n, 3) f32, normals (n, 3) f32 or None, cameras (V, 15) f64,
        images (V, H, W, C) f32, depths (V, H, W) f32 or None -> colors (>= n, C) f32, weight
        [>= n] f32, views [>= n] int32 (the bits of the u32 mask); mode 0: blend, 1: best."""
        n = len(points)
        V = _table(cameras, 15, torch.float64, "cameras", align=8)
        _, H, W, C = _stack(images, V, "images", channels=True)
        _chk(points, torch.float32, 3 * n, "points")
        _chk(normals, torch.float32, 3 * n, "normals", optional=True)
        _chk(depths, torch.float32, V * H * W, "depths", optional=True)
        _chk(colors, torch.float32, n * C, "colors")
        _chk(weight, torch.float32, n, "weight")
        _chk(views, torch.int32, n, "views")
        self._check(self.lib.rn_project_colors(
            self._h, n, _ptr(points), _ptr(normals), V, _ptr(cameras), H, W, C, _ptr(images),
            _ptr(depths), float(tol), float(min_cos), float(border), int(mode), _ptr(colors),
            _ptr(weight), _ptr(views), _stream()))

    # ---- depth maps into a TSDF volume (raynet_amd/fusion.py) --------------------------------
    def tsdf_integrate(self, cameras, depths, weights, trunc, border, tsdf=None, weight=None):
        """rn_tsdf_integrate: cameras (V, 15) f64, depths (V, H, W) f32 of distances to the camera
        centres, weights (V, H, W) f32 or None -> (tsdf, weight), both [gx][gy][gz] f32 over the
        context's grid: the weighted mean of the views' truncated signed distances (in units of
        `trunc`, 1 in free space) and the sum of their weights; 1 and 0 where no view counts."""
        V, H, W = _stack(depths, None, "depths")
        if weights is not None and _stack(weights, V, "weights") != (V, H, W):
            raise ValueError("weights: expected the shape of depths %s, got %s"
                             % ((V, H, W), tuple(weights.shape)))
        _table(cameras, 15, torch.float64, "cameras", align=8, rows=V)
        if tsdf is None:
            tsdf = torch.empty(self.grid_shape, dtype=torch.float32, device=depths.device)
        if weight is None:
            weight = torch.empty(self.grid_shape, dtype=torch.float32, device=depths.device)
        _chk(tsdf, torch.float32, self.G, "tsdf")
        _chk(weight, torch.float32, self.G, "weight")
        self._check(self.lib.rn_tsdf_integrate(
            self._h, V, _ptr(cameras), H, W, _ptr(depths), _ptr(weights), float(trunc),
            float(border), _ptr(tsdf), _ptr(weight), _stream()))
        return tsdf, weight

    # ---- the other views' verdict on points (raynet_amd/consistency.py) -----------------------
    def points_consistency(self, points, cameras, depths, exclude, tol_abs, tol_rel, border,
                           seen=None, agree=None, violate=None, residual=None):
        """rn_points_consistency: points (3, n) f64, cameras (V, 15) f64, depths (V, H, W) f32 of
        distances to the camera centres, 1 <= V <= 32, exclude: the view that is skipped or -1 ->
        (seen, agree, violate, residual): three [n] int32 (the bits of the u32 masks, bit v for
        view v: it measures something at the point's pixel / agrees with the point within
        tol_abs + tol_rel * depth / sees past the point) and [n] f32, the mean signed distance
        over the agreeing views, 0 where none agrees."""
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[0] != 3:
            raise ValueError("points: expected shape (3, n), got %s"
                             % (tuple(getattr(points, "shape", ())),))
        n = int(points.shape[1])
        _chk(points, torch.float64, 3 * n, "points", align=8)
        V, H, W = _stack(depths, None, "depths")
        if not 1 <= V <= 32:
            raise ValueError("depths: 1 to 32 views (a bit of the masks each), got %d" % V)
        _table(cameras, 15, torch.float64, "cameras", align=8, rows=V)
        exclude = int(exclude)
        if not -1 <= exclude < V:
            raise ValueError("exclude: a view 0..%d or -1, got %d" % (V - 1, exclude))
        outs = []
        for t, name, dtype in ((seen, "seen", torch.int32), (agree, "agree", torch.int32),
                               (violate, "violate", torch.int32),
                               (residual, "residual", torch.float32)):
            if t is None:
                t = torch.empty((n,), dtype=dtype, device=points.device)
            outs.append(_chk(t, dtype, n, name))
        self._check(self.lib.rn_points_consistency(
            self._h, n, _ptr(points), V, _ptr(cameras), H, W, _ptr(depths), exclude,
            float(tol_abs), float(tol_rel), float(border), _ptr(outs[0]), _ptr(outs[1]),
            _ptr(outs[2]), _ptr(outs[3]), _stream()))
        return tuple(outs)

    # ---- which views to use (raynet_amd/view_selection.py) -----------------------------------
    def view_overlap(self, points, normals, cameras, image_shape, depths, tol, min_cos, border,
                     cos_lo, cos_hi, visible=None, pairs=None):
        """rn_view_overlap: points (3, n) f64, normals (3, n) f64 or None, cameras (V, 15) f64,
        1 <= V <= 64, image_shape (H, W), depths (V, H, W) f32 or None, the band of the
        triangulation angle as cosines 0 <= cos_lo <= cos_hi <= 1 -> (visible, pairs): [n] int64
        (the bits of the u64 masks, bit v: view v sees the point) and (V, V) int64, which is ADDED
        to -- the points every view sees on the diagonal, the points two views share above it; a
        fresh one is zeroed here, a given one is the caller's."""
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[0] != 3:
            raise ValueError("points: expected shape (3, n), got %s"
                             % (tuple(getattr(points, "shape", ())),))
        n = int(points.shape[1])
        _chk(points, torch.float64, 3 * n, "points", align=8)
        if normals is not None:
            if not isinstance(normals, torch.Tensor) or tuple(normals.shape) != (3, n):
                raise ValueError("normals: expected shape (3, %d), got %s"
                                 % (n, tuple(getattr(normals, "shape", ())),))
            _chk(normals, torch.float64, 3 * n, "normals", align=8)
        V = _table(cameras, 15, torch.float64, "cameras", align=8)
        if not 1 <= V <= 64:
            raise ValueError("cameras: 1 to 64 views (a bit of the mask each), got %d" % V)
        H, W = (int(s) for s in image_shape)
        if depths is not None and _stack(depths, V, "depths") != (V, H, W):
            raise ValueError("depths: expected %s, got %s" % ((V, H, W), tuple(depths.shape)))
        if visible is None:
            visible = torch.empty((n,), dtype=torch.int64, device=points.device)
        if pairs is None:
            pairs = torch.zeros((V, V), dtype=torch.int64, device=points.device)
        _chk(visible, torch.int64, n, "visible", align=8)
        if tuple(pairs.shape) != (V, V):
            raise ValueError("pairs: expected %s, got %s" % ((V, V), tuple(pairs.shape)))
        _chk(pairs, torch.int64, V * V, "pairs", align=8)
        self._check(self.lib.rn_view_overlap(
            self._h, n, _ptr(points), _ptr(normals), V, _ptr(cameras), H, W, _ptr(depths),
            float(tol), float(min_cos), float(border), float(cos_lo), float(cos_hi),
            _ptr(visible), _ptr(pairs), _stream()))
        return visible, pairs

    def view_gain(self, visible, V, chosen, redundancy, gain=None):
        """rn_view_gain: visible [n] int64 (the bits of rn_view_overlap's masks), V views, chosen:
        the 64-bit mask of the views taken so far (a Python int, any 64 bits), redundancy 1..64 ->
        gain [V + 1] int64, which is ADDED to (a fresh one is zeroed here): per view not in chosen
        the number of points that fewer than `redundancy` chosen views see and that it sees; at V
        the number of such points."""
        V, redundancy = int(V), int(redundancy)
        if not 1 <= V <= 64:
            raise ValueError("V: 1 to 64 views, got %d" % V)
        if not 1 <= redundancy <= 64:
            raise ValueError("redundancy: 1 to 64, got %d" % redundancy)
        if not isinstance(visible, torch.Tensor) or visible.dim() != 1:
            raise ValueError("visible: expected shape (n,), got %s"
                             % (tuple(getattr(visible, "shape", ())),))
        n = int(visible.shape[0])
        _chk(visible, torch.int64, n, "visible", align=8)
        if gain is None:
            gain = torch.zeros((V + 1,), dtype=torch.int64, device=visible.device)
        _chk(gain, torch.int64, V + 1, "gain", align=8)
        chosen = int(chosen) & 0xFFFFFFFFFFFFFFFF
        if chosen >= 1 << 63:
            chosen -= 1 << 64                   # the same 64 bits as an int64_t
        self._check(self.lib.rn_view_gain(self._h, n, _ptr(visible), V, chosen, redundancy,
                                          _ptr(gain), _stream()))
        return gain

    # ---- connected components of a mesh (raynet_amd/components.py) ---------------------------
    def mesh_components(self, faces, n_vertices, labels=None, vertex_counts=None, face_counts=None):
        """rn_mesh_components: faces (nf, 3) i32 of a mesh with `n_vertices` vertices -> (labels,
        vertex_counts, face_counts), each [nv] i32: the smallest vertex index of every vertex's
        component (two vertices are connected if a face names both), and at every label the
        numbers of its vertices and of its faces (0 elsewhere).  A face with an index outside
        [0, nv) connects and counts nothing.  Synchronises the stream once (the status word comes
        back: RaynetHipError if the union-find reached a bound, which no input can cause)."""
        nv = int(n_vertices)
        if nv < 0:
            raise ValueError("n_vertices: 0 or more, got %d" % nv)
        nf = _table(faces, 3, torch.int32, "faces")
        outs = []
        for t, name in ((labels, "labels"), (vertex_counts, "vertex_counts"),
                        (face_counts, "face_counts")):
            if t is None:
                t = torch.empty((nv,), dtype=torch.int32, device=faces.device)
            outs.append(_chk(t, torch.int32, nv, name))
        status = torch.zeros((1,), dtype=torch.int32, device=faces.device)
        self._check(self.lib.rn_mesh_components(self._h, nv, nf, _ptr(faces), _ptr(outs[0]),
                                                _ptr(outs[1]), _ptr(outs[2]), _ptr(status),
                                                _stream()))
        if int(status.item()) != 0:
            raise _lib.RaynetHipError("rn_mesh_components: a pointer chase reached its bound "
                                      "(nv %d, nf %d): the labels are not to be used" % (nv, nf))
        return tuple(outs)

    # ---- Taubin smoothing of a mesh (raynet_amd/smoothing.py) ---------------------------------
    def mesh_smooth_workspace_bytes(self, nv, nf):
        """rn_mesh_smooth_workspace_bytes: the bytes rn_mesh_smooth needs for nv vertices, nf faces."""
        return _size(self.lib.rn_mesh_smooth_workspace_bytes(self._h, int(nv), int(nf)),
                     "rn_mesh_smooth_workspace_bytes", nv=nv, nf=nf)

    def mesh_smooth(self, vertices, faces, offsets, corners, fixed=None, iterations=10, lam=0.5,
                    mu=-0.53, max_move=float("inf"), workspace=None, out=None):
        """rn_mesh_smooth: vertices (nv, 3) f32, faces (nf, 3) i32, the corner table (offsets
        [nv + 1] i32, corners [3 nf] i32), fixed [nv] u8 or None -> (nv, 3) f32: `iterations`
        Taubin iterations (a step with `lam`, then one with `mu` unless it is 0), no coordinate
        farther than `max_move` from where it started.  workspace: a uint8 tensor of at least
        mesh_smooth_workspace_bytes(nv, nf) bytes, 8-byte aligned (allocated if None)."""
        nv, nf = _chk_mesh(vertices, faces, offsets, corners)
        _chk(fixed, torch.uint8, nv, "fixed", optional=True, align=1)
        need = self.mesh_smooth_workspace_bytes(nv, nf)
        workspace = _workspace(workspace, need, vertices.device)
        if out is None:
            out = torch.empty((nv, 3), dtype=torch.float32, device=vertices.device)
        _chk(out, torch.float32, 3 * nv, "out")
        self._check(self.lib.rn_mesh_smooth(
            self._h, nv, _ptr(vertices), nf, _ptr(faces), _ptr(offsets), _ptr(corners), _ptr(fixed),
            int(iterations), float(lam), float(mu), float(max_move), _ptr(workspace), _ptr(out),
            _stream()))
        return out

    # ---- vertex clustering of a mesh (raynet_amd/simplify.py) ----------------------------------
    def mesh_simplify_workspace_bytes(self, nv, nf, dims):
        """rn_mesh_simplify_workspace_bytes: the bytes rn_mesh_simplify needs for nv vertices, nf
        faces and a grid of dims[0] x dims[1] x dims[2] cells (32 bytes per cell)."""
        d = _host3(dims, ctypes.c_int32, "dims")
        return _size(self.lib.rn_mesh_simplify_workspace_bytes(int(nv), int(nf), d),
                     "rn_mesh_simplify_workspace_bytes", nv=nv, nf=nf, dims=tuple(d))

    def mesh_simplify(self, vertices, faces, origin, cell, dims, workspace=None):
        """rn_mesh_simplify: vertices (nv, 3) f32, faces (nf, 3) i32, the grid (origin [3], cell
        [3] > 0, dims [3] >= 1 on the host) -> (vertices_out (nv', 3) f32, faces_out (nf', 3) i32,
        source [nv'] i32, cluster [nv] i32): the vertices that share a cell become one at their
        mean, faces with two corners in one cluster and vertices no face is left for vanish.
        workspace: a uint8 tensor of at least mesh_simplify_workspace_bytes(nv, nf, dims) bytes,
        8-byte aligned (allocated if None).  Synchronises the stream once: the two counts come
        back to slice the outputs."""
        nv, nf = _chk_mesh(vertices, faces)
        d = _host3(dims, ctypes.c_int32, "dims")
        o = _host3(origin, ctypes.c_double, "origin")
        c = _host3(cell, ctypes.c_double, "cell")
        need = self.mesh_simplify_workspace_bytes(nv, nf, dims)
        workspace = _workspace(workspace, need, vertices.device)
        device = vertices.device
        vertices_out = torch.empty((nv, 3), dtype=torch.float32, device=device)
        faces_out = torch.empty((nf, 3), dtype=torch.int32, device=device)
        source = torch.empty((nv,), dtype=torch.int32, device=device)
        cluster = torch.empty((nv,), dtype=torch.int32, device=device)
        counts = torch.empty((2,), dtype=torch.int64, device=device)
        self._check(self.lib.rn_mesh_simplify(
            self._h, nv, _ptr(vertices), nf, _ptr(faces), o, c, d, _ptr(vertices_out),
            _ptr(faces_out), _ptr(source), _ptr(cluster), _ptr(counts), _ptr(workspace), _stream()))
        nv_out, nf_out = (int(x) for x in counts.tolist())
        return vertices_out[:nv_out], faces_out[:nf_out], source[:nv_out], cluster

    # ---- quadric-error placement of the clustered vertices (raynet_amd/simplify.py) -------------
    def mesh_place_quadric_workspace_bytes(self, nv, nf, nvo):
        """rn_mesh_place_quadric_workspace_bytes: the bytes rn_mesh_place_quadric needs for nv
        input vertices, nf input faces and nvo output vertices (88 per output vertex)."""
        return _size(self.lib.rn_mesh_place_quadric_workspace_bytes(int(nv), int(nf), int(nvo)),
                     "rn_mesh_place_quadric_workspace_bytes", nv=nv, nf=nf, nvo=nvo)

    def mesh_place_quadric(self, vertices, faces, cluster, positions, cell, regularization=2.0 ** -10,
                           max_move=1.0, workspace=None, out=None):
        """rn_mesh_place_quadric: the input mesh of mesh_simplify (vertices (nv, 3) f32, faces
        (nf, 3) i32), its `cluster` [nv] i32 and its output vertices `positions` (nvo, 3) f32, the
        sides of a cell (cell [3] > 0 on the host) -> (positions_out (nvo, 3) f32, counts [2]
        int64 on the host): every output vertex at the minimiser of its summed squared distances to
        the planes of the faces around its cluster, `regularization` in [2^-20, 1] pulling it to
        `positions`, no coordinate farther than `max_move` cell sides from there; counts: the
        vertices whose bits changed, the vertices of two or more members that kept theirs because
        the placement was refused.  workspace: a uint8 tensor of at least
        mesh_place_quadric_workspace_bytes(nv, nf, nvo) bytes, 8-byte aligned (allocated if None).
        One read-back: the counts."""
        nv, nf = _chk_mesh(vertices, faces)
        _chk(cluster, torch.int32, nv, "cluster")
        nvo = _table(positions, 3, torch.float32, "positions")
        if nvo > nv:
            raise ValueError("positions: at most the %d rows of vertices, got %d" % (nv, nvo))
        c = _host3(cell, ctypes.c_double, "cell")
        need = self.mesh_place_quadric_workspace_bytes(nv, nf, nvo)
        workspace = _workspace(workspace, need, vertices.device)
        if out is None:
            out = torch.empty((nvo, 3), dtype=torch.float32, device=vertices.device)
        _chk(out, torch.float32, 3 * nvo, "out")
        counts = torch.empty((2,), dtype=torch.int64, device=vertices.device)
        self._check(self.lib.rn_mesh_place_quadric(
            self._h, nv, _ptr(vertices), nf, _ptr(faces), _ptr(cluster), nvo, _ptr(positions), c,
            float(regularization), float(max_move), _ptr(out), _ptr(counts), _ptr(workspace),
            _stream()))
        return out, counts.cpu().numpy()

    # ---- small holes of a mesh capped (raynet_amd/holes.py) ------------------------------------
    def mesh_fill_holes_workspace_bytes(self, nv, nf):
        """rn_mesh_fill_holes_workspace_bytes: the bytes rn_mesh_fill_holes needs for nv vertices
        and nf faces."""
        return _size(self.lib.rn_mesh_fill_holes_workspace_bytes(int(nv), int(nf)),
                     "rn_mesh_fill_holes_workspace_bytes", nv=nv, nf=nf)

    def mesh_fill_holes(self, vertices, faces, offsets, corners, max_edges, workspace=None):
        """rn_mesh_fill_holes: vertices (nv, 3) f32, faces (nf, 3) i32, the corner table (offsets
        [nv + 1] i32, corners [3 nf] i32), max_edges in 3..65536 -> (new_vertices (k, 3) f32,
        new_faces (m, 3) i32, source [k] i32, counts [5] int64 on the host): every simple boundary
        loop of at most max_edges edges gets a vertex at the mean of its vertices (new_vertices,
        index nv + its row) and a fan of faces; source: the loops' smallest vertices; counts:
        filled loops, new faces, loops, loops not simple, boundary half-edges.  workspace: a uint8
        tensor of at least mesh_fill_holes_workspace_bytes(nv, nf) bytes, 8-byte aligned
        (allocated if None).  One read-back: the counts come back to slice the outputs."""
        nv, nf = _chk_mesh(vertices, faces, offsets, corners)
        need = self.mesh_fill_holes_workspace_bytes(nv, nf)
        workspace = _workspace(workspace, need, vertices.device)
        device = vertices.device
        new_vertices = torch.empty((nf, 3), dtype=torch.float32, device=device)
        new_faces = torch.empty((3 * nf, 3), dtype=torch.int32, device=device)
        source = torch.empty((nf,), dtype=torch.int32, device=device)
        counts = torch.empty((5,), dtype=torch.int64, device=device)
        self._check(self.lib.rn_mesh_fill_holes(
            self._h, nv, _ptr(vertices), nf, _ptr(faces), _ptr(offsets), _ptr(corners),
            int(max_edges), _ptr(new_vertices), _ptr(new_faces), _ptr(source), _ptr(counts),
            _ptr(workspace), _stream()))
        counts = counts.cpu().numpy()
        k, m = int(counts[0]), int(counts[1])
        return new_vertices[:k], new_faces[:m], source[:k], counts

    # -- timing (bench.py): hipEvents on the stream the kernels run on ------
    def timer_start(self):
        self._check(self.lib.rn_timer_start(self._h, _stream()))

    def timer_stop(self):
        ms = ctypes.c_float()
        self._check(self.lib.rn_timer_stop(self._h, _stream(), ctypes.byref(ms)))
        return float(ms.value)

    # ---- differentiable MRF block (training) -----------------------------------------
    def _chk_api_rows(self, rvi, rvc, *float_rows):
        """K-API layouts: rvi [n][M][3] i32, rvc [n] i32, float rows [n][M] f32."""
        n = len(rvc)
        _chk(rvi, torch.int32, n * self.M * 3, "ray_voxel_indices")
        _chk(rvc, torch.int32, n, "ray_voxel_count")
        for k, t in enumerate(float_rows):
            _chk(t, torch.float32, n * self.M, "row array %d" % k, optional=True)
        return n

    def plane_weights(self, rvi, rvc, starts, ends, left, c1, c2):
        n = self._chk_api_rows(rvi, rvc, c1, c2)
        _chk(left, torch.int32, n * self.M, "left")
        _chk(starts, torch.float32, 3 * n, "starts", align=4)
        _chk(ends, torch.float32, 3 * n, "ends", align=4)
        self._check(self.lib.rn_plane_weights(self._h, len(rvc), _ptr(rvi), _ptr(rvc), _ptr(starts),
                                              _ptr(ends), _ptr(left), _ptr(c1), _ptr(c2),
                                              _stream()))

    def train_bp_sweep(self, Sr, rvi, rvc, acc_in, msgs_in, acc_out, msgs_out):
        self._chk_api_rows(rvi, rvc, Sr, msgs_in, msgs_out)
        _chk(acc_in, torch.float32, self.G, "acc_in"); _chk(acc_out, torch.float32, self.G, "acc_out")
        self._check(self.lib.rn_train_bp_sweep(self._h, len(rvc), _ptr(Sr), _ptr(rvi), _ptr(rvc),
                                               _ptr(acc_in), _ptr(msgs_in), _ptr(acc_out),
                                               _ptr(msgs_out), _stream()))

    def train_depth(self, Sr, rvi, rvc, acc, msgs, S_new):
        self._chk_api_rows(rvi, rvc, Sr, msgs, S_new)
        _chk(acc, torch.float32, self.G, "acc")
        self._check(self.lib.rn_train_depth(self._h, len(rvc), _ptr(Sr), _ptr(rvi), _ptr(rvc),
                                            _ptr(acc), _ptr(msgs), _ptr(S_new), _stream()))

    def train_bp_sweep_bwd(self, Sr, rvi, rvc, acc_in, msgs_in, g_msgs_out, g_acc_out, g_Sr,
                           g_acc_in, g_msgs_in):
        self._chk_api_rows(rvi, rvc, Sr, msgs_in, g_msgs_out, g_Sr, g_msgs_in)
        for name, t in (("acc_in", acc_in), ("g_acc_out", g_acc_out), ("g_acc_in", g_acc_in)):
            _chk(t, torch.float32, self.G, name)
        self._check(self.lib.rn_train_bp_sweep_bwd(
            self._h, len(rvc), _ptr(Sr), _ptr(rvi), _ptr(rvc), _ptr(acc_in), _ptr(msgs_in),
            _ptr(g_msgs_out), _ptr(g_acc_out), _ptr(g_Sr), _ptr(g_acc_in), _ptr(g_msgs_in),
            _stream()))

    def train_depth_bwd(self, Sr, rvi, rvc, acc, msgs, g_S_new, g_Sr, g_acc, g_msgs):
        self._chk_api_rows(rvi, rvc, Sr, msgs, g_S_new, g_Sr, g_msgs)
        _chk(acc, torch.float32, self.G, "acc"); _chk(g_acc, torch.float32, self.G, "g_acc")
        self._check(self.lib.rn_train_depth_bwd(
            self._h, len(rvc), _ptr(Sr), _ptr(rvi), _ptr(rvc), _ptr(acc), _ptr(msgs),
            _ptr(g_S_new), _ptr(g_Sr), _ptr(g_acc), _ptr(g_msgs), _stream()))

    # ---- consumers of the depth maps (point clouds, metrics) --------------------------
    @staticmethod
    def _chk_view(H, W, camera, n_camera, center, depth_map, name):
        """One view of the float64 kernels: a [3][4] / [4][3] matrix, a centre of FOUR components
        (both kernels read center[3]) and an (H, W) f32 depth map."""
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise ValueError("H, W: at least 1 and H * W below 2^31, got %d, %d" % (H, W))
        _chk(camera, torch.float64, n_camera, name, align=8)
        _chk(center, torch.float64, 4, "center", align=8)
        _chk(depth_map, torch.float32, H * W, "depth_map")
        return H, W

    def depthmap_points(self, H, W, P_pinv, center, depth_map, points):
        """P_pinv [4][3] f64, center [4] f64, depth_map (H, W) f32 -> points (3, H*W) f64, the
        point of pixel (v, u) at column u*H + v."""
        H, W = self._chk_view(H, W, P_pinv, 12, center, depth_map, "P_pinv")
        _chk(points, torch.float64, 3 * H * W, "points", align=8)
        self._check(self.lib.rn_depthmap_points(self._h, H, W, _ptr(P_pinv), _ptr(center),
                                                _ptr(depth_map), _ptr(points), _stream()))

    def consistency_tau(self, H, W, first, points, P, center, depth_map, tau):
        """points (3, n) f64, P [3][4] f64, center [4] f64, depth_map (H, W) f32, tau [n] f64
        (read unless `first`, written)."""
        H, W = self._chk_view(H, W, P, 12, center, depth_map, "P")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[0] != 3:
            raise ValueError("points: expected shape (3, n), got %s"
                             % (tuple(getattr(points, "shape", ())),))
        n = int(points.shape[1])
        _chk(points, torch.float64, 3 * n, "points", align=8)
        _chk(tau, torch.float64, n, "tau", align=8)
        self._check(self.lib.rn_consistency_tau(self._h, n, H, W, 1 if first else 0, _ptr(points),
                                                _ptr(P), _ptr(center), _ptr(depth_map), _ptr(tau),
                                                _stream()))

    def nearest_neighbors(self, ref_xyzw, query_xyzw, dist, idx=None):
        """ref_xyzw (n_ref, 4) f32, query_xyzw (n_query, 4) f32 (the fourth lane is not read) ->
        dist [n_query] f32 and / or idx [n_query] i32 (either may be None, not both)."""
        n_ref = _table(ref_xyzw, 4, torch.float32, "ref_xyzw", align=16)
        n_query = _table(query_xyzw, 4, torch.float32, "query_xyzw", align=16)
        if dist is None and idx is None:
            raise ValueError("dist, idx: at least one output is required")
        _chk(dist, torch.float32, n_query, "dist", optional=True)
        _chk(idx, torch.int32, n_query, "idx", optional=True)
        self._check(self.lib.rn_nearest_neighbors(self._h, n_ref, _ptr(ref_xyzw), n_query,
                                                  _ptr(query_xyzw), _ptr(dist), _ptr(idx),
                                                  _stream()))

    # ---- point-cloud filters (raynet_amd/metrics.py: VoxelMask, ReduceDensity) ------------
    def voxel_mask(self, points, box, mask, keep):
        """points (3, n) f64, box [12] f64 (min | max | step | step / 2), mask (A, B, C) u8."""
        n = points.shape[1]
        A, B, C = (int(s) for s in mask.shape)
        _chk(points, torch.float64, 3 * n, "points", align=8)
        _chk(box, torch.float64, 12, "box", align=8)
        _chk(mask, torch.uint8, A * B * C, "mask", align=1)
        _chk(keep, torch.uint8, n, "keep", align=1)
        self._check(self.lib.rn_voxel_mask(self._h, n, _ptr(points), _ptr(box), A, B, C,
                                           _ptr(mask), _ptr(keep), _stream()))

    def thin_keys(self, points, lo, h, seed, position, keys, priority):
        """Cell keys and visiting priorities of points (3, n) f64; position: None or [n] i64."""
        n = points.shape[1]
        _chk(points, torch.float64, 3 * n, "points", align=8)
        _chk(position, torch.int64, n, "position", optional=True, align=8)
        _chk(keys, torch.int64, n, "keys", align=8)
        _chk(priority, torch.int64, n, "priority", align=8)
        self._check(self.lib.rn_thin_keys(self._h, n, _ptr(points), float(lo[0]), float(lo[1]),
                                          float(lo[2]), float(h), int(seed), _ptr(position),
                                          _ptr(keys), _ptr(priority), _stream()))

    def thin_round(self, work, sorted_keys, points, priority, index, r2, state, undecided):
        """One round over `work` (None: all points) of the arrays in key order."""
        n = points.shape[1]
        n_work = n if work is None else work.shape[0]
        _chk(work, torch.int32, n_work, "work", optional=True)
        _chk(sorted_keys, torch.int64, n, "sorted_keys", align=8)
        _chk(points, torch.float64, 3 * n, "points", align=8)
        _chk(priority, torch.int64, n, "priority", align=8)
        _chk(index, torch.int32, n, "index")
        _chk(state, torch.int32, n, "state")
        _chk(undecided, torch.int32, 1, "undecided")
        self._check(self.lib.rn_thin_round(self._h, n_work, _ptr(work), n, _ptr(sorted_keys),
                                           _ptr(points), _ptr(priority), _ptr(index), float(r2),
                                           _ptr(state), _ptr(undecided), _stream()))

    # ---- ground-truth depth from a point cloud (raynet_amd/cloud_depth.py) ---------------
    def cloud_zbuffer(self, points, cameras, H, W, zbuf, counts=None):
        """points (n, 3) f32, cameras (V, 21) f64 (K | R | t), zbuf (V, H, W) i32 holding float
        bit patterns, filled with 0x7F800000 by the caller; counts: None or [2] i64, zeroed
        (landed pairs | atomics the pre-test skipped)."""
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError("H, W: at least 1, got %d, %d" % (H, W))
        n = _table(points, 3, torch.float32, "points")
        V = _table(cameras, 21, torch.float64, "cameras", align=8)
        if n > (1 << 30):
            raise ValueError("points: at most 2^30 per call, got %d" % n)
        _chk(zbuf, torch.int32, V * H * W, "zbuf")
        if counts is None:
            self._check(self.lib.rn_cloud_zbuffer(self._h, n, _ptr(points), V, _ptr(cameras), H, W,
                                                  _ptr(zbuf), _stream()))
        else:
            _chk(counts, torch.int64, 2, "counts", align=8)
            self._check(self.lib.rn_cloud_zbuffer_counted(self._h, n, _ptr(points), V,
                                                          _ptr(cameras), H, W, _ptr(zbuf),
                                                          _ptr(counts), _stream()))

    # ---- training batches of rays from many reference views (train_network/ray_sampler.py) ---
    BATCH_CAMERA_FLOATS = 28      # P_pinv [4][3] | centre [4] | P [3][4]

    def _chk_batch_tables(self, view, nbr, n):
        _chk(view, torch.int32, n, "view")
        if nbr.dim() != 2 or not 1 <= nbr.shape[1] <= 16:
            raise ValueError("nbr: expected shape (V, N) with 1 <= N <= 16, got %s" % (tuple(nbr.shape),))
        V, N = int(nbr.shape[0]), int(nbr.shape[1])
        _chk(nbr, torch.int32, V * N, "nbr")
        return V, N

    def batch_rays(self, view, ray_idxs, depth, cams, nbr, patch_shape, points, target, centres,
                   flags, sampling=None):
        """rn_batch_rays: n candidate rays, each of its own reference view, in one launch.
        view, ray_idxs [n] i32, depth [n] f32, cams (V, 28) f32, nbr (V, N) i32 -> points
        [n, D, 4], target [n, 4], centres [n, N, D, 2] i32, flags [n] i32 (0 = valid).  An index
        out of range raises (the entry decides it from the kernel's own tests and synchronises).
        sampling: an rn_sampling POD (HipContext.sampling) -> rn_batch_rays_scheme; the far view of
        sample_in_disparity is cams[nbr[view][N - 1]], the POD's is not read."""
        n = len(ray_idxs)
        V, N = self._chk_batch_tables(view, nbr, n)
        h, w = int(patch_shape[0]), int(patch_shape[1])
        if h < 1 or w < 1:
            raise ValueError("patch_shape: at least 1 x 1, got %s" % (tuple(patch_shape),))
        if n * N * self.D >= 1 << 30:
            raise ValueError("n * N * D = %d: at most 2^30 per call" % (n * N * self.D))
        _chk(ray_idxs, torch.int32, n, "ray_idxs")
        _chk(depth, torch.float32, n, "depth")
        _table(cams, self.BATCH_CAMERA_FLOATS, torch.float32, "cams", rows=V)
        _chk(points, torch.float32, n * self.D * 4, "points", align=16)
        _chk(target, torch.float32, n * 4, "target", align=16)
        _chk(centres, torch.int32, n * N * self.D * 2, "centres", align=8)
        _chk(flags, torch.int32, n, "flags")
        if sampling is not None:
            self._check(self.lib.rn_batch_rays_scheme(
                self._h, n, _ptr(view), _ptr(ray_idxs), _ptr(depth), _ptr(cams), V, _ptr(nbr), N, h,
                w, ctypes.byref(sampling), _ptr(points), _ptr(target), _ptr(centres), _ptr(flags),
                _stream()))
            return
        self._check(self.lib.rn_batch_rays(self._h, n, _ptr(view), _ptr(ray_idxs), _ptr(depth),
                                           _ptr(cams), V, _ptr(nbr), N, h, w, _ptr(points),
                                           _ptr(target), _ptr(centres), _ptr(flags), _stream()))

    def batch_patches(self, images, view, centres, nbr, patch_shape, patches):
        """rn_batch_patches: images (V, H, W, C) f32, view [n], centres [n, N, D, 2], nbr (V, N)
        -> patches (N, n, D, h, w, C) f32, zero outside the images."""
        n = len(view)
        V, N = self._chk_batch_tables(view, nbr, n)
        h, w = int(patch_shape[0]), int(patch_shape[1])
        if h < 1 or w < 1:
            raise ValueError("patch_shape: at least 1 x 1, got %s" % (tuple(patch_shape),))
        if images.dim() != 4 or tuple(images.shape[:3]) != (V, self.H, self.W):
            raise ValueError("images: expected shape (%d, %d, %d, C), got %s"
                             % (V, self.H, self.W, tuple(images.shape)))
        C = int(images.shape[3])
        if self.D * h * w * C >= 1 << 30 or self.H * self.W * C >= 1 << 31:
            raise ValueError("patches of %d x %d x %d x %d floats per ray and view: too large"
                             % (self.D, h, w, C))
        _chk(images, torch.float32, V * self.H * self.W * C, "images")
        _chk(centres, torch.int32, n * N * self.D * 2, "centres", align=8)
        _chk(patches, torch.float32, N * n * self.D * h * w * C, "patches")
        self._check(self.lib.rn_batch_patches(self._h, n, _ptr(images), V, C, _ptr(view),
                                              _ptr(centres), _ptr(nbr), N, h, w, _ptr(patches),
                                              _stream()))

    KERNEL_NAMES = {1: "traverse", 2: "sweep_map", 3: "bp", 4: "depth", 5: "acc", 6: "other", 7: "scatter"}

    # ---- ground truth from scene meshes (raynet_amd/mesh.py) ----------------------------
    def mesh_keys(self, triangles, box, keys):
        n = triangles.shape[0]
        _chk(triangles, torch.float32, 9 * n, "triangles")
        _chk(box, torch.float32, 6, "box")
        _chk(keys, torch.int64, n, "keys", align=8)
        self._check(self.lib.rn_mesh_keys(self._h, n, _ptr(triangles), _ptr(box), _ptr(keys),
                                          _stream()))

    def mesh_build(self, triangles, sorted_keys, nodes, leaves, work):
        """Leaves, hierarchy and node boxes; returns the tree's depth (synchronises)."""
        n = triangles.shape[0]
        _chk(triangles, torch.float32, 9 * n, "triangles")
        _chk(sorted_keys, torch.int64, n, "sorted_keys", align=8)
        _chk(nodes, torch.float32, 16 * max(n - 1, 1), "nodes", align=16)
        _chk(leaves, torch.float32, 12 * n, "leaves", align=16)
        _chk(work, torch.uint8, 56 * n + 64, "work", align=16)
        depth = ctypes.c_int32(0)
        self._check(self.lib.rn_mesh_build(self._h, n, _ptr(triangles), _ptr(sorted_keys),
                                           _ptr(nodes), _ptr(leaves), _ptr(work),
                                           ctypes.byref(depth), _stream()))
        return int(depth.value)

    def mesh_raycast(self, origins, destinations, nodes, leaves, points, tri):
        n = origins.shape[0]
        for name, t in (("origins", origins), ("destinations", destinations), ("points", points)):
            _chk(t, torch.float32, 3 * n, name)
        _chk(tri, torch.int32, n, "tri")
        _chk(nodes, torch.float32, 16, "nodes", align=16)
        _chk(leaves, torch.float32, 12, "leaves", align=16)
        self._check(self.lib.rn_mesh_raycast(self._h, n, _ptr(origins), _ptr(destinations),
                                             _ptr(nodes), _ptr(leaves), _ptr(points), _ptr(tri),
                                             _stream()))

    def mesh_closest(self, queries, nodes, leaves, dist, closest=None, tri=None):
        n = queries.shape[0]
        _chk(queries, torch.float64, 3 * n, "queries", align=8)
        _chk(dist, torch.float64, n, "dist", align=8)
        _chk(closest, torch.float64, 3 * n, "closest", optional=True, align=8)
        _chk(tri, torch.int32, n, "tri", optional=True)
        _chk(nodes, torch.float32, 16, "nodes", align=16)
        _chk(leaves, torch.float32, 12, "leaves", align=16)
        self._check(self.lib.rn_mesh_closest(self._h, n, _ptr(queries), _ptr(nodes), _ptr(leaves),
                                             _ptr(dist), _ptr(closest), _ptr(tri), _stream()))

    def mesh_areas(self, triangles, area):
        n = triangles.shape[0]
        _chk(triangles, torch.float32, 9 * n, "triangles")
        _chk(area, torch.float64, n, "area", align=8)
        self._check(self.lib.rn_mesh_areas(self._h, n, _ptr(triangles), _ptr(area), _stream()))

    def mesh_sample(self, triangles, area_cdf, seed, points, tri):
        n, T = tri.shape[0], triangles.shape[0]
        _chk(triangles, torch.float32, 9 * T, "triangles")
        _chk(area_cdf, torch.float64, T, "area_cdf", align=8)
        _chk(points, torch.float32, 3 * n, "points")
        _chk(tri, torch.int32, n, "tri")
        self._check(self.lib.rn_mesh_sample(self._h, n, T, _ptr(triangles), _ptr(area_cdf),
                                            int(seed), _ptr(points), _ptr(tri), _stream()))

    def mesh_depthmap(self, H, W, P_pinv, center, nodes, leaves, depth_map):
        _chk(P_pinv, torch.float32, 12, "P_pinv")
        _chk(center, torch.float32, 3, "center")
        _chk(nodes, torch.float32, 16, "nodes", align=16)
        _chk(leaves, torch.float32, 12, "leaves", align=16)
        _chk(depth_map, torch.float32, int(H) * int(W), "depth_map")
        self._check(self.lib.rn_mesh_depthmap(self._h, int(H), int(W), _ptr(P_pinv), _ptr(center),
                                              _ptr(nodes), _ptr(leaves), _ptr(depth_map),
                                              _stream()))

    # ---- a mesh seen from cameras (raynet_amd/render.py) ---------------------------------------
    def mesh_render(self, nodes, leaves, vertices, faces, cameras, H, W, colors=None, normals=None):
        """rn_mesh_render: the BVH (nodes, leaves) of the triangles vertices[faces], vertices
        (nv, 3) f32, faces (nf, 3) i32, cameras (V, 15) f32 rows P_pinv | centre, optional colors
        (nv, C) f32 with C in 1..4 and normals (nv, 3) f32 -> (face (V, H, W) i32, depth (V, H, W)
        f32, bary (V, H, W, 2) f32, color (V, H, W, C) f32 or None, normal (V, H, W, 3) f32 or
        None): per pixel the face hit first (-1: none), the distance of the hit to the centre, its
        Moeller-Trumbore (u, v) and the attributes interpolated there; 0 on a miss."""
        nv, nf = _chk_mesh(vertices, faces)
        H, W = int(H), int(W)
        V = _table(cameras, 15, torch.float32, "cameras")
        _chk(nodes, torch.float32, 16 * max(nf - 1, 1), "nodes", align=16)
        _chk(leaves, torch.float32, 12 * nf, "leaves", align=16)
        C = 0
        if colors is not None:
            if colors.dim() != 2 or colors.shape[0] != nv or not 1 <= colors.shape[1] <= 4:
                raise ValueError("colors: expected (%d, C) with C in 1..4, got %s"
                                 % (nv, tuple(colors.shape)))
            C = int(colors.shape[1])
            _chk(colors, torch.float32, nv * C, "colors")
        if normals is not None:
            _table(normals, 3, torch.float32, "normals", rows=nv)
        device = vertices.device
        face = torch.empty((V, H, W), dtype=torch.int32, device=device)
        depth = torch.empty((V, H, W), dtype=torch.float32, device=device)
        bary = torch.empty((V, H, W, 2), dtype=torch.float32, device=device)
        color = None if colors is None else torch.empty((V, H, W, C), dtype=torch.float32,
                                                        device=device)
        normal = None if normals is None else torch.empty((V, H, W, 3), dtype=torch.float32,
                                                          device=device)
        self._check(self.lib.rn_mesh_render(
            self._h, _ptr(nodes), _ptr(leaves), nv, _ptr(vertices), nf, _ptr(faces), _ptr(colors),
            C, _ptr(normals), V, _ptr(cameras), H, W, _ptr(face), _ptr(depth), _ptr(bary),
            _ptr(color), _ptr(normal), _stream()))
        return face, depth, bary, color, normal

    # ---- a texture atlas from the photographs (raynet_amd/texture.py) --------------------------
    def texture_bake(self, vertices, faces, normals, T, cells_per_row, cameras, images, depths, tol,
                     min_cos, border, mode, texture, weight, views):
        """rn_texture_bake: vertices (nv, 3) f32, faces (nf, 3) i32, normals (nv, 3) f32 or None,
        cameras (V, 15) f64, images (V, H, W, C) f32, depths (V, H, W) f32 or None -> texture
        (>= Ht, Wt, C) f32, weight (>= Ht, Wt) f32, views (>= Ht, Wt) int32 (the bits of the u32
        mask) of the atlas of T steps per leg and cells_per_row cells per row; mode 0: blend, 1:
        best."""
        nv, nf = _chk_mesh(vertices, faces)
        T, Cw = int(T), int(cells_per_row)
        V = _table(cameras, 15, torch.float64, "cameras", align=8)
        _, H, W, C = _stack(images, V, "images", channels=True)
        texels = _atlas_texels(nf, T, Cw)
        _chk(normals, torch.float32, 3 * nv, "normals", optional=True)
        _chk(depths, torch.float32, V * H * W, "depths", optional=True)
        _chk(texture, torch.float32, texels * C, "texture")
        _chk(weight, torch.float32, texels, "weight")
        _chk(views, torch.int32, texels, "views")
        self._check(self.lib.rn_texture_bake(
            self._h, nv, _ptr(vertices), nf, _ptr(faces), _ptr(normals), T, Cw, V, _ptr(cameras),
            H, W, C, _ptr(images), _ptr(depths), float(tol), float(min_cos), float(border),
            int(mode), _ptr(texture), _ptr(weight), _ptr(views), _stream()))

    def texture_sample(self, face, bary, n_faces, T, cells_per_row, texture, bilinear, color):
        """rn_texture_sample: face [n] i32 and bary (n, 2) f32 (rn_mesh_render's planes,
        flattened), texture (Ht, Wt, C) f32 of the atlas of n_faces faces -> color (>= n, C) f32:
        the atlas at every pixel's place in its face's chart, bilinear or the nearest texel; 0
        where the pixel sees no face."""
        n = int(face.numel())
        if texture.dim() != 3 or not 1 <= texture.shape[2] <= 4:
            raise ValueError("texture: expected (Ht, Wt, C) with C in 1..4, got %s"
                             % (tuple(texture.shape),))
        C = int(texture.shape[2])
        nf, T, Cw = int(n_faces), int(T), int(cells_per_row)
        texels = _atlas_texels(nf, T, Cw)
        _chk(face, torch.int32, n, "face")
        _chk(bary, torch.float32, 2 * n, "bary")
        _chk(texture, torch.float32, texels * C, "texture")
        _chk(color, torch.float32, n * C, "color")
        self._check(self.lib.rn_texture_sample(self._h, n, _ptr(face), _ptr(bary), nf, T, Cw, C,
                                               _ptr(texture), 1 if bilinear else 0, _ptr(color),
                                               _stream()))

    def prof_begin(self, capacity=4096, only=None):
        """only: kernel family names to bracket (None = all of them)."""
        mask = 0xFFFFFFFF
        if only is not None:
            ids = {v: k for k, v in self.KERNEL_NAMES.items()}
            mask = 0
            for name in only:
                mask |= 1 << ids[name]
        self._check(self.lib.rn_prof_select(self._h, mask))
        self._prof_cap = capacity
        self.prof_active = True
        self._check(self.lib.rn_prof_begin(self._h, capacity))

    def prof_end(self):
        """-> list of (kernel name, n_rays, milliseconds), one per launch."""
        cap = self._prof_cap
        self.prof_active = False
        ids = (ctypes.c_int32 * cap)()
        rays = (ctypes.c_int32 * cap)()
        ms = (ctypes.c_float * cap)()
        n = ctypes.c_int32()
        self._check(self.lib.rn_prof_end(self._h, ctypes.byref(n), ids, rays, ms))
        starts = (ctypes.c_float * cap)()
        self._check(self.lib.rn_prof_offsets(self._h, starts))
        self.prof_starts = [float(starts[i]) for i in range(n.value)]
        return [(self.KERNEL_NAMES.get(ids[i], str(ids[i])), int(rays[i]), float(ms[i]))
                for i in range(n.value)]

    def selftest_arith(self, a, out):
        """out[2][n]: roundf(a), round_half_away(a) (tests only)."""
        self._check(self.lib.rn_selftest_arith(self._h, a.numel(), _ptr(a), _ptr(out), _stream()))

    def selftest_quotient(self, x, d, out):
        """out[3][n]: round_half_away(x / d), round_quotient_fast's value, sure (tests only)."""
        self._check(self.lib.rn_selftest_quotient(self._h, x.numel(), _ptr(x), _ptr(d), _ptr(out),
                                                  _stream()))

    def selftest_feature_offsets(self, P, starts, ends, out):
        """out [n][N][D][2] int32: feature-vector index per ray / view / plane by the generic
        and by the cooperative sweep's index arithmetic (tests only)."""
        self._check(self.lib.rn_selftest_feature_offsets(self._h, len(starts), _ptr(P), _ptr(starts),
                                                         _ptr(ends), _ptr(out), _stream()))

    def selftest_mapping(self, a, b, t, out):
        """out[5][n]: a / b, Markstein's quotient, usable, the walk's plane index, the table's
        (tests only)."""
        self._check(self.lib.rn_selftest_mapping(self._h, a.numel(), _ptr(a), _ptr(b), _ptr(t),
                                                 _ptr(out), _stream()))

    # -- thin wrappers; argument order is the header's ------------------------
    def fill_f32(self, t, value):
        self._check(self.lib.rn_fill_f32(self._h, _ptr(t), t.numel(), float(value), _stream()))

    def fill_i32(self, t, value):
        self._check(self.lib.rn_fill_i32(self._h, _ptr(t), t.numel(), int(value), _stream()))

    def sample_rays(self, ray_idxs, P_inv, center, starts, ends):
        self._check(self.lib.rn_sample_rays(self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(P_inv),
                                            _ptr(center), _ptr(starts), _ptr(ends), _stream()))

    def sample_points(self, ray_idxs, P_inv, center, points):
        self._check(self.lib.rn_sample_points(self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(P_inv),
                                              _ptr(center), _ptr(points), _stream()))

    def compute_similarities(self, features, P, starts, ends, S):
        self._check(self.lib.rn_compute_similarities(self._h, len(starts), _ptr(features), _ptr(P),
                                                     _ptr(starts), _ptr(ends), _ptr(S), _stream()))

    def voxel_traversal(self, starts, ends, rvi, rvc):
        self._check(self.lib.rn_voxel_traversal(self._h, len(starts), _ptr(starts), _ptr(ends),
                                                _ptr(rvi), _ptr(rvc), _stream()))

    def planes_to_voxels(self, rvi, rvc, starts, ends, S, S_new):
        self._check(self.lib.rn_planes_to_voxels(self._h, len(rvc), _ptr(rvi), _ptr(rvc),
                                                 _ptr(starts), _ptr(ends), _ptr(S), _ptr(S_new),
                                                 _stream()))

    def bp_sweep(self, S, rvi, rvc, acc_in, msgs_in, acc_out, msgs_out):
        self._check(self.lib.rn_bp_sweep(self._h, len(rvc), _ptr(S), _ptr(rvi), _ptr(rvc),
                                         _ptr(acc_in), _ptr(msgs_in), _ptr(acc_out),
                                         _ptr(msgs_out), _stream()))

    def depth_estimation(self, S, rvi, rvc, acc, msgs, S_new):
        self._check(self.lib.rn_depth_estimation(self._h, len(rvc), _ptr(S), _ptr(rvi), _ptr(rvc),
                                                 _ptr(acc), _ptr(msgs), _ptr(S_new), _stream()))

    def mvcnn_similarities(self, ray_idxs, features, P, P_inv, center, S):
        self._check(self.lib.rn_mvcnn_similarities(self._h, len(ray_idxs), _ptr(ray_idxs),
                                                   _ptr(features), _ptr(P), _ptr(P_inv),
                                                   _ptr(center), _ptr(S), _stream()))

    def mvcnn_depth(self, ray_idxs, features, P, P_inv, center, S, points, depth_map):
        self._check(self.lib.rn_mvcnn_depth(self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(features),
                                            _ptr(P), _ptr(P_inv), _ptr(center), _ptr(S),
                                            _ptr(points), _ptr(depth_map), _stream()))

    # -- K8 / K9 / K10 and the batch assembler under a sampling scheme (rn_sampling) ---------
    @staticmethod
    def sampling(scheme="sample_in_bbox", depth_range=None, far_view=None, far_from_table=False):
        """The rn_sampling POD.  scheme: a name of _lib.SAMPLING_SCHEMES (or its id);
        depth_range (r0, r1) for sample_in_range; far_view = (P 3x4, P_pinv 4x3, centre) of the
        LAST view of the ray's neighbour list for sample_in_disparity (host arrays) --
        far_from_table: for batch_rays, which reads it out of its camera table."""
        sm = _lib.Sampling()
        if isinstance(scheme, str):
            if scheme not in _lib.SAMPLING_SCHEMES:
                raise NotImplementedError(scheme)
            scheme = _lib.SAMPLING_SCHEMES[scheme]
        sm.scheme = int(scheme)
        if sm.scheme == _lib.SAMPLING_SCHEMES["sample_in_range"] and depth_range is None:
            raise ValueError("sample_in_range needs a depth_range (r0, r1)")
        if depth_range is not None:
            sm.range[0], sm.range[1] = float(depth_range[0]), float(depth_range[1])
        if sm.scheme == _lib.SAMPLING_SCHEMES["sample_in_disparity"] and far_view is None \
                and not far_from_table:
            raise ValueError("sample_in_disparity needs the far view (P, P_pinv, centre)")
        if far_view is not None:
            P, P_inv, centre = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a,
                                           np.float32).ravel() for a in far_view)
            if P.size != 12 or P_inv.size != 12 or centre.size not in (3, 4):
                raise ValueError("far_view: (P 3x4, P_pinv 4x3, centre 3 or 4)")
            sm.far_P[:] = P.tolist()
            sm.far_P_inv[:] = P_inv.tolist()
            sm.far_centre[:] = (centre.tolist() + [1.0])[:4]
        return sm

    def sample_points_scheme(self, ray_idxs, P_inv, center, sampling, points):
        n = len(ray_idxs)
        _chk(ray_idxs, torch.int32, n, "ray_idxs")
        _chk(P_inv, torch.float32, 12, "P_inv")
        _chk(center, torch.float32, 3, "center")
        _chk(points, torch.float32, n * self.D * 4, "points", align=16)
        self._check(self.lib.rn_sample_points_scheme(self._h, n, _ptr(ray_idxs), _ptr(P_inv),
                                                     _ptr(center), ctypes.byref(sampling),
                                                     _ptr(points), _stream()))

    def _chk_sweep(self, n, ray_idxs, features, P, P_inv, center, S):
        _chk(ray_idxs, torch.int32, n, "ray_idxs")
        _chk(features, torch.float32,
             self.N * (self.H + self.padding + 1) * (self.W + self.padding + 1) * self.F, "features",
             align=16)
        _chk(P, torch.float32, 12 * self.N, "P")
        _chk(P_inv, torch.float32, 12, "P_inv")
        _chk(center, torch.float32, 3, "center")
        _chk(S, torch.float32, n * self.D, "S")

    def mvcnn_similarities_scheme(self, ray_idxs, features, P, P_inv, center, sampling, S):
        n = len(ray_idxs)
        self._chk_sweep(n, ray_idxs, features, P, P_inv, center, S)
        self._check(self.lib.rn_mvcnn_similarities_scheme(
            self._h, n, _ptr(ray_idxs), _ptr(features), _ptr(P), _ptr(P_inv), _ptr(center),
            ctypes.byref(sampling), _ptr(S), _stream()))

    def mvcnn_depth_scheme(self, ray_idxs, features, P, P_inv, center, sampling, S, points,
                           depth_map):
        n = len(ray_idxs)
        self._chk_sweep(n, ray_idxs, features, P, P_inv, center, S)
        _chk(points, torch.float32, n * self.D * 4, "points", align=16)
        _chk(depth_map, torch.float32, n, "depth_map")
        self._check(self.lib.rn_mvcnn_depth_scheme(
            self._h, n, _ptr(ray_idxs), _ptr(features), _ptr(P), _ptr(P_inv), _ptr(center),
            ctypes.byref(sampling), _ptr(S), _ptr(points), _ptr(depth_map), _stream()))

    def mvcnn_voxel_space(self, ray_idxs, features, P, P_inv, center, rvi, rvc, S_voxel,
                          depth_map=None):
        if depth_map is None:
            self._check(self.lib.rn_mvcnn_voxel_space(
                self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(features), _ptr(P), _ptr(P_inv),
                _ptr(center), _ptr(rvi), _ptr(rvc), _ptr(S_voxel), _stream()))
        else:
            self._check(self.lib.rn_mvcnn_voxel_space_depth(
                self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(features), _ptr(P), _ptr(P_inv),
                _ptr(center), _ptr(rvi), _ptr(rvc), _ptr(S_voxel), _ptr(depth_map), _stream()))

    def fused_bp_sweep(self, ray_idxs, features, P, P_inv, center, rvi, rvc, S_voxel, acc_in,
                       msgs_in, acc_out, msgs_out):
        self._check(self.lib.rn_fused_bp_sweep(
            self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(features), _ptr(P), _ptr(P_inv),
            _ptr(center), _ptr(rvi), _ptr(rvc), _ptr(S_voxel), _ptr(acc_in), _ptr(msgs_in),
            _ptr(acc_out), _ptr(msgs_out), _stream()))

    def fused_depth(self, ray_idxs, features, P, P_inv, center, rvi, rvc, S_voxel, acc, msgs,
                    depth_map):
        self._check(self.lib.rn_fused_depth(
            self._h, len(ray_idxs), _ptr(ray_idxs), _ptr(features), _ptr(P), _ptr(P_inv),
            _ptr(center), _ptr(rvi), _ptr(rvc), _ptr(S_voxel), _ptr(acc), _ptr(msgs),
            _ptr(depth_map), _stream()))

    # -- resident-scene path ---------------------------------------------------
    def _segments(self, rows):
        """Scratch for the rays' bbox entry / exit points ([rows][8] f32), kept per context."""
        seg = self._seg_scratch
        if seg is None or seg.shape[0] < rows:
            seg = torch.empty((rows, 8), dtype=torch.float32, device=self.device)
            self._seg_scratch = seg
        return seg

    def scene_prepare(self, ray_idxs, feature_views, P, P_inv, center, vox, rvc, Sr, order=None):
        assert len(feature_views) == self.N
        n = len(ray_idxs)
        f32, i32 = torch.float32, torch.int32
        fdim = self.feature_shape[1] * self.feature_shape[2] * self.F
        for k, fv in enumerate(feature_views):
            _chk(fv, f32, fdim, "feature map %d" % k, align=16)
        _chk(ray_idxs, i32, n, "ray_idxs"); _chk(order, i32, n, "order", optional=True)
        _chk(P, f32, 12 * self.N, "P"); _chk(P_inv, f32, 12, "P_inv")
        _chk(center, f32, 3, "center")
        ra = self._row_align
        _chk(vox, i32, n * self.M, "vox", align=ra); _chk(rvc, i32, n, "rvc")
        _chk(Sr, f32, n * self.M, "Sr", align=ra)
        assert order is None or len(order) == n
        arr = (ctypes.c_void_p * self.N)(*[fv.data_ptr() for fv in feature_views])
        self._check(self.lib.rn_scene_prepare(self._h, n, _ptr(ray_idxs), arr, _ptr(P),
                                              _ptr(P_inv), _ptr(center), _ptr(order), _ptr(vox),
                                              _ptr(rvc), _ptr(Sr),
                                              _ptr(self._segments(n)), _stream()))

    def _chk_scene(self, n_images, rows_per_image, ray_idxs, feature_table, cameras, vox, rvc, Sr,
                   order):
        """What scene_prepare_all and a scene plan take alike: feature_table, an int64 CUDA tensor
        [n_images, N] of device pointers; cameras, float32 [n_images, 12N + 16]; the rays and
        their schedule [n]; the row arrays of all images -> (n, rows)."""
        n, rows = len(ray_idxs), int(n_images) * int(rows_per_image)
        f32, i32, ra = torch.float32, torch.int32, self._row_align
        _chk(feature_table, torch.int64, n_images * self.N, "feature_table", align=8)
        assert tuple(feature_table.shape) == (n_images, self.N)
        _chk(cameras, f32, n_images * (12 * self.N + 16), "cameras")
        assert tuple(cameras.shape) == (n_images, 12 * self.N + 16)
        _chk(ray_idxs, i32, n, "ray_idxs"); _chk(order, i32, n, "order", optional=True)
        _chk(vox, i32, rows * self.M, "vox", align=ra); _chk(rvc, i32, rows, "rvc")
        _chk(Sr, f32, rows * self.M, "Sr", align=ra)
        return n, rows

    def scene_prepare_all(self, n_images, rows_per_image, ray_idxs, feature_table, cameras, vox,
                          rvc, Sr, order=None):
        """feature_table, cameras: see _chk_scene."""
        n, rows = self._chk_scene(n_images, rows_per_image, ray_idxs, feature_table, cameras, vox,
                                  rvc, Sr, order)
        assert order is None or len(order) == n
        self._check(self.lib.rn_scene_prepare_all(
            self._h, int(n_images), n, int(rows_per_image), _ptr(ray_idxs),
            _ptr(feature_table), _ptr(cameras), _ptr(order), _ptr(vox), _ptr(rvc), _ptr(Sr),
            _ptr(self._segments(rows)), _stream()))

    def scene_plan(self, n_images, rows_per_image, ray_idxs, feature_table, cameras, vox, rvc, Sr,
                   msgs, acc0, acc1, depth, prior, patch_rows, acc_fixed=None, order=None,
                   depth_image=None, sweep_xcd_chunk=0, stats=None, stats_image=None):
        """An rn_scene_plan over the caller's buffers, every tensor validated ONCE here; the
        returned object (which keeps them alive) goes to scene_run.  depth_image [n_images, R]:
        the depth sweeps write the maps in ray-index (pixel) order there instead of `depth`.
        stats [3, rows] / stats_image [3, n_images, R]: the depth sweeps also write confidence,
        expected depth and depth std (rn_scene_depth_stats) next to the depths -- in row order,
        or, with depth_image, in pixel order."""
        assert rows_per_image % 256 == 0 and len(ray_idxs) <= rows_per_image
        n, rows = self._chk_scene(n_images, rows_per_image, ray_idxs, feature_table, cameras, vox,
                                  rvc, Sr, order)
        f32 = torch.float32
        _chk(msgs, f32, rows * self.M, "msgs", align=self._row_align)
        _chk(depth, f32, rows, "depth")
        G = self.acc_size()
        _chk(acc0, f32, G, "acc[0]", align=16); _chk(acc1, f32, G, "acc[1]", align=16)
        _chk(acc_fixed, torch.int64, G, "acc_fixed", optional=True, align=16)
        seg = self._segments(rows)
        pl = _lib.ScenePlan()
        pl.n_images, pl.n, pl.rows_per_image = int(n_images), n, int(rows_per_image)
        pl.ray_idxs, pl.order = ray_idxs.data_ptr(), (order.data_ptr() if order is not None else None)
        pl.features_views, pl.cameras = feature_table.data_ptr(), cameras.data_ptr()
        pl.vox, pl.rvc, pl.Sr, pl.msgs = vox.data_ptr(), rvc.data_ptr(), Sr.data_ptr(), msgs.data_ptr()
        pl.ray_segments = seg.data_ptr()
        pl.acc[0], pl.acc[1] = acc0.data_ptr(), acc1.data_ptr()
        pl.acc_fixed = acc_fixed.data_ptr() if acc_fixed is not None else None
        pl.depth, pl.prior = depth.data_ptr(), float(prior)
        pl.row_layout = 1 if patch_rows else 0
        pl.depth_image, pl.depth_image_stride = None, 0
        assert sweep_xcd_chunk >= 0 and sweep_xcd_chunk % 4 == 0
        pl.sweep_xcd_chunk = int(sweep_xcd_chunk)
        if depth_image is not None:
            assert depth_image.dim() == 2 and depth_image.shape[0] == n_images
            _chk(depth_image, f32, depth_image.numel(), "depth_image")
            if n:       # every ray index is a valid entry of an image's map (checked once, here)
                lo, hi = int(ray_idxs.min()), int(ray_idxs.max())
                assert 0 <= lo and hi < depth_image.shape[1], (lo, hi, tuple(depth_image.shape))
            pl.depth_image, pl.depth_image_stride = depth_image.data_ptr(), int(depth_image.shape[1])
        pl.stats, pl.stats_image, pl.stats_image_stride = None, None, 0
        if stats is not None:
            assert tuple(stats.shape) == (3, rows), tuple(stats.shape)
            _chk(stats, f32, 3 * rows, "stats")
            pl.stats = stats.data_ptr()
        if stats_image is not None:
            assert depth_image is not None and \
                tuple(stats_image.shape) == (3,) + tuple(depth_image.shape), tuple(stats_image.shape)
            _chk(stats_image, f32, 3 * depth_image.numel(), "stats_image")
            pl.stats_image = stats_image.data_ptr()
            pl.stats_image_stride = int(depth_image.numel())
        # (the tensors the struct points into live as long as it does.  No `byref(pl)` is kept ON
        # pl: that is a reference cycle through a ctypes object the collector does not track --
        # every plan ever built, with its 7 GB of buffers, stayed allocated: round 6)
        pl._keepalive = (ray_idxs, feature_table, cameras, vox, rvc, Sr, msgs, acc0, acc1, depth,
                         acc_fixed, order, seg, depth_image, stats, stats_image)
        return pl

    def scene_run(self, plan, phases, iteration=0, image=-1):
        """rn_scene_run: the phases (a mask of _lib.RN_RUN_*) of one pass, one C call."""
        self._check(self.lib.rn_scene_run(self._h, ctypes.byref(plan), int(phases), int(iteration),
                                          int(image), _stream()))

    def count_voxels(self, ray_idxs, cameras):
        """-> int32 [n_images, n]: voxels crossed by every ray of ray_idxs in every reference
        image (rn_scene_count_voxels; cameras as for scene_prepare_all)."""
        n_images, n = int(cameras.shape[0]), len(ray_idxs)
        _chk(cameras, torch.float32, n_images * (12 * self.N + 16), "cameras")
        _chk(ray_idxs, torch.int32, n, "ray_idxs")
        out = torch.zeros((n_images, n), dtype=torch.int32, device=self.device)
        self._check(self.lib.rn_scene_count_voxels(self._h, n_images, n, _ptr(ray_idxs),
                                                   _ptr(cameras), _ptr(out), _stream()))
        return out

    def _chk_rows(self, Sr, vox, rvc, msgs, acc, part=None, part_dtype=torch.float32):
        n = len(rvc)
        f32, i32 = torch.float32, torch.int32
        ra = self._row_align
        _chk(Sr, f32, n * self.M, "Sr", align=ra); _chk(vox, i32, n * self.M, "vox", align=ra)
        _chk(rvc, i32, n, "rvc")
        _chk(msgs, f32, n * self.M, "msgs", align=ra)
        _chk(acc, f32, self.acc_size(), "accumulator", align=16)
        if part is not None:
            _chk(part, part_dtype, self.acc_size(), "partial accumulator", align=16)
        return n

    def _bp_sweep(self, entry, part_dtype, Sr, vox, rvc, acc_in, msgs, acc_part, first_sweep,
                  patch_rows, uniform_acc):
        """rn_scene_bp_sweep or its fixed-point twin: they differ in the partial sums' type."""
        n = self._chk_rows(Sr, vox, rvc, msgs, acc_in, acc_part, part_dtype)
        # a work list bound for another tensor must not meet a launch whose buffer happens to sit
        # at the address (and have the row count) the list was built for: unbind unless `vox` IS
        # the tensor it describes
        items = self._scatter_items
        if items is not None and items[1] is not vox:
            self.bind_scatter_items(None)
        self._check(entry(self._h, n, _ptr(Sr), _ptr(vox), _ptr(rvc), _ptr(acc_in), _ptr(msgs),
                          _ptr(acc_part), (1 if first_sweep else 0) | (2 if uniform_acc else 0),
                          1 if patch_rows else 0, _stream()))

    def scene_bp_sweep(self, Sr, vox, rvc, acc_in, msgs, acc_part, first_sweep=False,
                       patch_rows=False, uniform_acc=False):
        self._bp_sweep(self.lib.rn_scene_bp_sweep, torch.float32, Sr, vox, rvc, acc_in, msgs,
                       acc_part, first_sweep, patch_rows, uniform_acc)

    def scene_bp_sweep_fixed(self, Sr, vox, rvc, acc_in, msgs, acc_part_fixed, first_sweep=False,
                             patch_rows=False, uniform_acc=False):
        self._bp_sweep(self.lib.rn_scene_bp_sweep_fixed, torch.int64, Sr, vox, rvc, acc_in, msgs,
                       acc_part_fixed, first_sweep, patch_rows, uniform_acc)

    def acc_combine_fixed(self, acc_part_fixed, prior, acc_out):
        _chk(acc_part_fixed, torch.int64, acc_out.numel(), "partial accumulator", align=16)
        _chk(acc_out, torch.float32, 1, "accumulator", align=16)
        assert acc_out.numel() == self.acc_size()
        self._check(self.lib.rn_acc_combine_fixed(self._h, _ptr(acc_part_fixed), float(prior),
                                                  _ptr(acc_out), _stream()))

    def acc_combine_fixed_range(self, part_fixed, prior, out):
        """fixed -> float on any slab: out[i] = prior + part_fixed[i] * 2^-32; zeroes the slab."""
        n = part_fixed.numel()
        _chk(part_fixed, torch.int64, n, "fixed-point slab", align=8)
        _chk(out, torch.float32, n, "accumulator slab")
        self._check(self.lib.rn_acc_combine_fixed_range(self._h, _ptr(part_fixed), n, float(prior),
                                                        _ptr(out), _stream()))

    def acc_combine(self, acc_part, prior, acc_out):
        _chk(acc_part, torch.float32, self.acc_size(), "partial accumulator")
        _chk(acc_out, torch.float32, self.acc_size(), "accumulator")
        self._check(self.lib.rn_acc_combine(self._h, _ptr(acc_part), float(prior), _ptr(acc_out),
                                            _stream()))

    def acc_reduce_local(self, acc_part, acc_out):
        _chk(acc_part, torch.float32, self.acc_size(), "partial accumulator")
        _chk(acc_out, torch.float32, self.acc_size(), "accumulator")
        self._check(self.lib.rn_acc_reduce_local(self._h, _ptr(acc_part), _ptr(acc_out), _stream()))

    def acc_add_prior(self, acc, prior):
        _chk(acc, torch.float32, self.acc_size(), "accumulator")
        self._check(self.lib.rn_acc_add_prior(self._h, _ptr(acc), float(prior), _stream()))

    def scene_depth(self, Sr, vox, rvc, acc, msgs, center, S_new, depth_map, rays_per_center=0):
        n = self._chk_rows(Sr, vox, rvc, msgs, acc)
        _chk(S_new, torch.float32, n * self.M, "S_new", optional=True)
        _chk(depth_map, torch.float32, n, "depth_map", optional=True)
        _chk_centers(center, n, rays_per_center, optional=depth_map is None)
        self._check(self.lib.rn_scene_depth(self._h, n, _ptr(Sr), _ptr(vox), _ptr(rvc),
                                            _ptr(acc), _ptr(msgs), _ptr(center),
                                            int(rays_per_center), _ptr(S_new), _ptr(depth_map),
                                            _stream()))

    def scene_depth_stats(self, Sr, vox, rvc, acc, msgs, center, S_new, depth_map, stats,
                          rays_per_center=0, stats_offset=0):
        """rn_scene_depth_stats: scene_depth plus stats [3, S] -- confidence, expected depth and
        depth std of every ray's distribution, ray i at stats[:, stats_offset + i].  depth_map and
        stats are required."""
        n = self._chk_rows(Sr, vox, rvc, msgs, acc)
        _chk(S_new, torch.float32, n * self.M, "S_new", optional=True)
        _chk(depth_map, torch.float32, n, "depth_map")
        _chk(stats, torch.float32, 3 * n, "stats")
        stats_offset = int(stats_offset)
        if stats.dim() != 2 or stats.shape[0] != 3 or stats_offset < 0 or \
                stats_offset + n > stats.shape[1]:
            raise ValueError("stats: expected shape (3, >= %d), got %s"
                             % (stats_offset + n, tuple(stats.shape)))
        _chk_centers(center, n, rays_per_center)
        self._check(self.lib.rn_scene_depth_stats(self._h, n, _ptr(Sr), _ptr(vox), _ptr(rvc),
                                                  _ptr(acc), _ptr(msgs), _ptr(center),
                                                  int(rays_per_center), _ptr(S_new),
                                                  _ptr(depth_map),
                                                  ctypes.c_void_p(stats.data_ptr() + 4 * stats_offset),
                                                  int(stats.shape[1]), _stream()))
