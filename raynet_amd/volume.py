"""The occupancy volume of the MRF: what the model believes about every voxel after a pass.

`RayNetForwardPass.occupancy_volume()` hands it out; here it is saved, loaded, turned into the
point cloud of its occupied voxels and rendered from any camera -- a reference image of the pass,
a held-out view, a camera that has no image at all.  The belief grid and
the rendering are HIP kernels (csrc/raynet_volume.inl, rn_occupancy_grid / rn_volume_render); the
voxel cloud is one pass of torch operations over the grid.

`OccupancyVolume.mesh()` is the surface of the volume: the iso-surface of the belief grid as an
indexed, closed, consistently oriented triangle mesh (`SurfaceMesh`; marching tetrahedra on the
GPU, csrc/raynet_isosurface.inl), which the mesh tools of the package take:
`MeshRaycaster`, its `sample_surface`, and through the sampled cloud the metrics.
"""

import numpy as np
import torch

from .appearance import check_face_indices
from .common.scene import get_voxel_grid

MAX_M = 1024        # rn_create's limit on the steps of a ray


class VolumeRender(object):
    """What `OccupancyVolume.render` returns: five (H, W) float32 maps in the orientation
    `forward_pass` returns depth maps in.  With o_i the belief of the i-th voxel a pixel's ray
    crosses, T_i = prod_{j<i} (1 - o_j), w_i = o_i T_i and t_i the distance of the voxel's centre
    from the camera (include/raynet_hip.h, rn_volume_render) --
      depth           t of the first voxel with the largest w
      opacity         1 - T behind the last voxel
      expected_depth  sum w_i t_i / sum w_i
      confidence      the largest w
      median_depth    t of the first voxel behind which T <= 1/2, 0 if the ray never gets there
    A pixel whose ray crosses no voxel has 0 everywhere."""
    __slots__ = ("depth", "opacity", "expected_depth", "confidence", "median_depth")
    FIELDS = __slots__

    def __init__(self, depth, opacity, expected_depth, confidence, median_depth):
        self.depth, self.opacity, self.expected_depth = depth, opacity, expected_depth
        self.confidence, self.median_depth = confidence, median_depth

    def __iter__(self):
        return iter(tuple(getattr(self, f) for f in self.FIELDS))


class SurfaceMesh(object):
    """An indexed triangle mesh: vertices (n, 3) float32, faces (m, 3) int32 rows of vertex
    indices, counter-clockwise seen from outside (host arrays; tensors are copied to the host).
    Optional per-vertex attributes: normals (n, 3) float32 (`compute_normals`) and colors (n, 3)
    uint8 (`colorize`); both go into the file when set."""

    def __init__(self, vertices, faces, normals=None, colors=None):
        if isinstance(vertices, torch.Tensor):
            vertices = vertices.detach().cpu().numpy()
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        faces = np.asarray(faces).reshape(-1, 3)
        check_face_indices(faces, len(self.vertices))
        self.faces = np.ascontiguousarray(faces, dtype=np.int32)
        self.normals = self.colors = None
        if normals is not None:
            self.normals = self._attribute(normals, np.float32, "normals")
        if colors is not None:
            self.colors = self._attribute(colors, np.uint8, "colors")

    def _attribute(self, values, dtype, name):
        a = np.ascontiguousarray(values, dtype=dtype)
        if a.shape != self.vertices.shape:
            raise ValueError("%s: expected %s, one row per vertex, got %s"
                             % (name, self.vertices.shape, a.shape))
        return a

    @property
    def empty(self):
        return len(self.faces) == 0

    def triangles(self):
        """[m, 9] float32 rows p0 | p1 | p2: what `MeshRaycaster` takes."""
        from .common.mesh_io import get_triangles
        return get_triangles(self.vertices, self.faces)

    def without_nonfinite(self):
        """-> a new SurfaceMesh without the faces that have a vertex with a non-finite component
        and without the vertices no remaining face names, renumbered; the order of faces and
        vertices is kept, normals and colours go along.  (The iso-surface of a field with NaN
        entries has such vertices: HipContext.isosurface, fusion.TSDFVolume.mesh.)"""
        from . import components
        finite = np.isfinite(self.vertices).all(1)
        return components.keep_faces(self, finite[self.faces].all(1))

    # ---- connected components (components.py) ------------------------
    def components(self):
        """-> components.MeshComponents: the pieces of the mesh -- two vertices are connected if
        a face names both (positions play no part) -- in the order of their smallest vertex, with
        their vertex and face counts."""
        from . import components
        if len(self.vertices) == 0:
            none = np.zeros(0, np.int32)
            return components.MeshComponents(none, none, none)
        return components.mesh_components(self.faces, len(self.vertices))

    def keep_components(self, ids_or_mask):
        """-> a new SurfaceMesh of the components named by `ids_or_mask` (dense ids of
        `components()`, or a boolean mask over them): their faces and the vertices those name,
        renumbered; the order of faces and vertices is kept, normals and colours go along."""
        from . import components
        if self.empty:
            return components.keep_faces(self, np.zeros(0, bool))
        found = self.components()
        which = np.asarray(ids_or_mask)
        if which.dtype == bool:
            if which.shape != (len(found),):
                raise ValueError("a mask over the components has %d entries, got %s"
                                 % (len(found), which.shape))
            keep = which
        else:
            ids = which.astype(np.int64).reshape(-1)
            if len(ids) and (ids.min() < 0 or ids.max() >= len(found)):
                raise ValueError("a component id outside 0..%d" % (len(found) - 1))
            keep = np.zeros(len(found), bool)
            keep[ids] = True
        return components.keep_faces(self, found.face_mask(self.faces, keep))

    def without_small_components(self, min_faces=None, min_fraction=None, keep_largest=None):
        """-> a new SurfaceMesh without the floaters: only the components stay that have at least
        `min_faces` faces, at least `min_fraction` of the largest component's faces, and are among
        the `keep_largest` largest by faces (ties to the one with the lower first vertex) --
        every criterion that is given.  Order, normals and colours as for `keep_components`."""
        from . import components
        return components.filter_small(self, min_faces, min_fraction, keep_largest)[0]

    # ---- small holes capped (holes.py) --------------------------------
    def filled(self, max_edges, return_stats=False):
        """-> a new SurfaceMesh with every simple boundary loop of 3..max_edges edges capped by a
        vertex at the mean of its vertices and a fan of faces (holes.fill_holes); with
        return_stats, (the mesh, the dict of the five counts).  This mesh's vertices and faces
        come first, in their order; a centre takes the colour of its loop's smallest vertex,
        normals are recomputed if and only if this mesh has them.  An empty mesh gives an empty
        mesh, without the GPU."""
        from . import holes
        if self.empty:
            holes.check_max_edges(max_edges)
            out = SurfaceMesh(self.vertices.copy(), self.faces.copy(), self.normals, self.colors)
            return (out, dict.fromkeys(holes.COUNTS, 0)) if return_stats else out
        vertices, faces, source, stats = holes.fill_holes(self.vertices, self.faces, max_edges)
        colors = None if self.colors is None else np.concatenate([self.colors, self.colors[source]])
        out = SurfaceMesh(vertices, faces, None, colors)
        if self.normals is not None:
            out.compute_normals()
        return (out, stats) if return_stats else out

    # ---- simplification (simplify.py) ---------------------------------
    def simplified(self, cell, origin=None, drop_duplicate_faces=True, placement="mean",
                   regularization=2.0 ** -10, max_move=1.0, return_stats=False):
        """-> a new SurfaceMesh with the vertices of every cell of a uniform grid (sides `cell`, a
        number or one per axis; simplify.simplify_mesh: the keywords are its own) merged at their
        mean, without the faces and vertices that vanish that way; with placement="quadric" the
        merged vertices lie where the planes of the faces around them meet (creases stay sharp)
        instead, `regularization` and `max_move` as in simplify_mesh.  Colours are those of each
        cluster's smallest vertex, normals are recomputed if and only if this mesh has them.  An
        empty mesh gives an empty mesh, without the GPU.  return_stats: (the mesh, simplify_mesh's
        dict of the placement)."""
        from . import simplify
        if self.empty:
            simplify.check_placement(placement, regularization, max_move)
            simplify.cluster_grid(self.vertices, cell, origin)
            out = SurfaceMesh(self.vertices.copy(), self.faces.copy(), self.normals, self.colors)
            return (out, {"moved": 0, "fell_back": 0, "farthest_move": 0.0}) if return_stats else out
        vertices, faces, source, stats = simplify.simplify_mesh(
            self.vertices, self.faces, cell, origin, drop_duplicate_faces, placement,
            regularization, max_move, True)
        out = SurfaceMesh(vertices, faces, None,
                          None if self.colors is None else self.colors[source])
        if self.normals is not None and out.empty:      # (everything in one cell)
            out.normals = np.zeros_like(out.vertices)
        elif self.normals is not None:
            out.compute_normals()
        return (out, stats) if return_stats else out

    # ---- smoothing (smoothing.py) -------------------------------------
    def smoothed(self, iterations=10, lam=0.5, mu=-0.53, fixed="boundary", max_move=None):
        """-> a new SurfaceMesh with the vertices after `iterations` Taubin iterations
        (smoothing.smooth_vertices: the keywords are its own): the terraces of an iso-surface and
        the noise of a fused surface flatten, the surface keeps its size.  The faces and their
        order stay, colours go along, normals are recomputed if and only if this mesh has them.
        An empty mesh gives an empty mesh, without the GPU."""
        from . import smoothing
        if self.empty:
            smoothing.check_parameters(iterations, float(lam), float(mu),
                                       float("inf") if max_move is None else float(max_move))
            return SurfaceMesh(self.vertices.copy(), self.faces.copy(), self.normals, self.colors)
        out = SurfaceMesh(smoothing.smooth_vertices(self.vertices, self.faces, iterations, lam, mu,
                                                    fixed, max_move),
                          self.faces.copy(), None, self.colors)
        if self.normals is not None:
            out.compute_normals()
        return out

    # ---- normals and colours (appearance.py) -------------------------
    def compute_normals(self):
        """Sets and returns `normals` (n, 3) float32: the unit area-weighted vertex normals,
        pointing outwards; (0, 0, 0) where the areas around a vertex cancel or it is in no face."""
        from .appearance import vertex_normals
        self.normals = vertex_normals(self.vertices, self.faces, unit=True)
        return self.normals

    def colorize(self, scene, frame_idxs, tol, min_cos=0.0, mode="blend", unseen=(0.5, 0.5, 0.5)):
        """Sets `colors` (n, 3) uint8 from the images of the scene's frames `frame_idxs` and
        returns the mask of the views that saw each vertex ([n] uint32, bit k: frame_idxs[k]).
        A frame sees a vertex that projects into its image, faces it (the vertex normal, computed
        if absent, at cos > min_cos) and is no farther from its camera than the mesh's own depth
        map there plus `tol` (scene units; a vertex lies on the surface it is tested against, so
        tol is the slack for the pixel's footprint -- a voxel diagonal is the natural size).  mode
        "blend": the cos^2-weighted mean of the frames, "best": the frame that faces the vertex
        best.  A vertex no frame sees gets `unseen`."""
        from .appearance import project_colors, scene_views, to_rgb8
        if self.empty:
            raise ValueError("the mesh is empty: there is no surface to colour")
        cameras, images = scene_views(scene, frame_idxs)
        H, W = np.asarray(images[0]).shape[:2]
        caster = self.raycaster()
        depth_maps = [caster.depth_map(cam, H, W) for cam in cameras]
        if self.normals is None:
            self.compute_normals()
        got = project_colors(self.vertices, cameras, images, depth_maps, self.normals, tol=tol,
                             min_cos=min_cos, mode=mode)
        self.colors = to_rgb8(got.colors, got.seen, unseen)
        return got.views

    # ---- which frames to take colours from (view_selection.py) ---------
    def best_frames(self, scene, frame_idxs, k, tol, min_cos=0.0, redundancy=1,
                    return_stats=False):
        """The (at most) k of the scene's frames `frame_idxs` (at most 64 candidates) that between
        them see the most vertices, in the order a greedy covering set chooses them: every round
        takes the frame that sees the most vertices fewer than `redundancy` chosen frames see yet,
        the earlier of equals, until k are taken or no frame adds anything.  A frame sees a vertex
        exactly as for `colorize`: it projects into the image, faces the frame (the vertex normal,
        computed if absent, at cos > min_cos) and is no farther from the camera than the mesh's
        own depth map there plus `tol`.  return_stats: -> (frames, gains, short), the vertices
        every frame added and the number still short at the end."""
        from .view_selection import MAX_VIEWS, view_overlap
        frame_idxs = [int(i) for i in frame_idxs]
        if self.empty:
            raise ValueError("the mesh is empty: there is no surface to choose frames for")
        if not 1 <= len(frame_idxs) <= MAX_VIEWS:
            raise ValueError("%d candidate frames: 1 to %d per call" % (len(frame_idxs), MAX_VIEWS))
        if int(k) < 0 or not 1 <= int(redundancy) <= MAX_VIEWS:
            raise ValueError("k: 0 or more, redundancy: 1 to %d, got %r, %r"
                             % (MAX_VIEWS, k, redundancy))
        cameras = [scene.get_image(i).camera for i in frame_idxs]
        H, W = scene.image_shape
        caster = self.raycaster()
        depth_maps = [caster.depth_map(cam, H, W) for cam in cameras]
        if self.normals is None:
            self.compute_normals()
        overlap = view_overlap(self.vertices, cameras, (H, W), normals=self.normals,
                               depth_maps=depth_maps, tol=tol, min_cos=min_cos)
        order, gains, short = overlap.cover(k, redundancy)
        chosen = [frame_idxs[v] for v in order]
        return (chosen, gains, short) if return_stats else chosen

    # ---- a texture atlas (texture.py) ---------------------------------
    def textured(self, scene, frame_idxs, T, tol, min_cos=0.0, mode="blend", normals="face"):
        """-> texture.MeshTexture: the images of the scene's frames `frame_idxs` (at most 32) baked
        into an atlas of T texel steps per chart leg.  The occluder is the mesh's own depth map
        per frame plus `tol`, exactly as for `colorize`; normals "face" tests a texel against its
        face's normal, "vertex" against the interpolated vertex normals (computed if absent)."""
        from .appearance import scene_views
        from .texture import bake_texture
        if self.empty:
            raise ValueError("the mesh is empty: there is no surface to texture")
        cameras, images = scene_views(scene, frame_idxs)
        H, W = np.asarray(images[0]).shape[:2]
        caster = self.raycaster()
        depth_maps = [caster.depth_map(cam, H, W) for cam in cameras]
        return bake_texture(self, cameras, images, T, depth_maps, tol=tol, min_cos=min_cos,
                            mode=mode, normals=normals)

    def save_obj(self, path, texture, unseen=(0.5, 0.5, 0.5)):
        """Writes STEM.obj (`v`, `vt`, `f a/ta b/tb c/tc`, 1-based, `mtllib` / `usemtl`), STEM.mtl
        (`map_Kd STEM.png`) and STEM.png beside it, STEM being `path` without its extension: the
        mesh with `texture` (texture.MeshTexture of this mesh's faces), texels no view saw in
        `unseen`.  Every face has three texture vertices of its own, in face order.  -> the three
        paths."""
        import os
        from .texture import face_uvs
        if texture.layout.n_faces != len(self.faces):
            raise ValueError("a texture of %d faces for a mesh of %d"
                             % (texture.layout.n_faces, len(self.faces)))
        stem = os.path.splitext(path)[0]
        name = os.path.basename(stem)
        obj, mtl, png = stem + ".obj", stem + ".mtl", stem + ".png"
        uvs = face_uvs(len(self.faces), texture.layout).reshape(-1, 2)
        with open(obj, "w") as f:
            f.write("# raynet_amd surface mesh\nmtllib %s.mtl\nusemtl %s\n" % (name, name))
            f.write("".join("v %.9g %.9g %.9g\n" % tuple(v) for v in self.vertices.tolist()))
            f.write("".join("vt %.17g %.17g\n" % tuple(t) for t in uvs.tolist()))
            f.write("".join("f %d/%d %d/%d %d/%d\n" % (a + 1, 3 * k + 1, b + 1, 3 * k + 2, c + 1,
                                                       3 * k + 3)
                            for k, (a, b, c) in enumerate(self.faces.tolist())))
        with open(mtl, "w") as f:
            f.write("newmtl %s\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd %s.png\n"
                    % (name, name))
        texture.save_png(png, unseen)
        return obj, mtl, png

    # ---- file ------------------------------------------------------------------------------
    def save_ply(self, path):
        """A binary little-endian PLY: `vertex` x y z float -- then nx ny nz float where the mesh
        has normals and red green blue uchar where it has colours -- and `face` one list
        vertex_indices of uchar 3 and three ints: the file common.mesh_io.parse_gt_data_from_ply
        reads back (and `load_ply` restores, attributes included)."""
        rows = np.empty((len(self.faces),), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        rows["n"] = 3
        rows["v"] = self.faces
        fields, header = [("xyz", "<f4", (3,))], ""
        if self.normals is not None:
            fields.append(("normal", "<f4", (3,)))
            header += "property float nx\nproperty float ny\nproperty float nz\n"
        if self.colors is not None:
            fields.append(("rgb", "u1", (3,)))
            header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        with open(path, "wb") as f:
            f.write(("ply\nformat binary_little_endian 1.0\ncomment raynet_amd surface mesh\n"
                     "element vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                     "%selement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                     % (len(self.vertices), header, len(self.faces))).encode())
            if len(fields) == 1:
                self.vertices.astype("<f4").tofile(f)
            else:
                table = np.empty((len(self.vertices),), dtype=fields)
                table["xyz"] = self.vertices
                if self.normals is not None:
                    table["normal"] = self.normals
                if self.colors is not None:
                    table["rgb"] = self.colors
                table.tofile(f)
            rows.tofile(f)

    @classmethod
    def load_ply(cls, path):
        from .common.mesh_io import parse_gt_data_from_ply, read_ply
        points, _, faces = parse_gt_data_from_ply(path)
        vertex = read_ply(path)["vertex"]
        normals = colors = None
        if all(k in vertex for k in ("nx", "ny", "nz")):
            normals = np.stack([vertex[k] for k in ("nx", "ny", "nz")], axis=1).astype(np.float32)
        if all(k in vertex for k in ("red", "green", "blue")):
            colors = np.stack([vertex[k] for k in ("red", "green", "blue")], axis=1).astype(np.uint8)
        return cls(points, faces, normals, colors)

    # ---- the mesh tools --------------------------------------------------------------------
    def raycaster(self):
        """-> raynet_amd.mesh.MeshRaycaster over the triangles (ray casting, closest points,
        area, sample_surface)."""
        if self.empty:
            raise ValueError("the mesh is empty: there is no surface to cast rays at or to sample")
        from .mesh import MeshRaycaster
        return MeshRaycaster(self.triangles())

    # ---- images of the surface (render.py) ----------------------------
    def render(self, cameras, H, W, raycaster=None):
        """-> render.MeshRender: per pixel of every camera the face hit first, its depth, where in
        the face, and this mesh's colours and normals (where it has them) interpolated there."""
        from .render import render_mesh
        return render_mesh(self, cameras, H, W, raycaster)

    def render_scene(self, scene, frame_idxs, raycaster=None):
        """`render` from the cameras of the scene's frames `frame_idxs`, at the scene's image
        size."""
        H, W = scene.image_shape
        return self.render([scene.get_image(int(i)).camera for i in frame_idxs], H, W, raycaster)

    def pointcloud(self, n_samples, seed=0):
        """-> raynet_amd.pointcloud.Pointcloud of `n_samples` area-weighted points of the
        surface (MeshRaycaster.sample_surface), for the point-cloud filters and the metrics."""
        if self.empty:
            raise ValueError("the mesh is empty: there is no surface to cast rays at or to sample")
        from .pointcloud import Pointcloud
        points, _ = self.raycaster().sample_surface(n_samples, seed)
        return Pointcloud(np.ascontiguousarray(points.cpu().numpy().T))


class OccupancyVolume(object):
    """belief: [gx][gy][gz] float32 occupancy probabilities (array or tensor, host or device);
    bbox: the 6 numbers of the scene's bounding box; grid_shape: (gx, gy, gz)."""

    KEYS = ("belief", "bbox", "grid_shape")

    def __init__(self, belief, bbox, grid_shape):
        self.grid_shape = tuple(int(g) for g in np.asarray(grid_shape).ravel())
        if len(self.grid_shape) != 3 or min(self.grid_shape) < 1:
            raise ValueError("grid_shape: three positive sizes, got %r" % (grid_shape,))
        self.bbox = np.ascontiguousarray(np.asarray(bbox, dtype=np.float32).reshape(-1))
        if self.bbox.shape != (6,):
            raise ValueError("bbox: 6 numbers, got %r" % (bbox,))
        if not isinstance(belief, torch.Tensor):
            belief = torch.from_numpy(np.ascontiguousarray(belief, dtype=np.float32))
        if belief.dtype != torch.float32 or tuple(belief.shape) != self.grid_shape:
            raise ValueError("belief: expected float32 of shape %s, got %s of shape %s"
                             % (self.grid_shape, belief.dtype, tuple(belief.shape)))
        self.belief = belief.contiguous()

    # ---- file ------------------------------------------------------------------------------
    def save(self, path):
        """An .npz of `belief` [gx][gy][gz] f32, `bbox` [6] f32 and `grid_shape` [3] i32."""
        with open(path, "wb") as f:        # (a file object: savez appends no suffix of its own)
            np.savez(f, belief=self.belief.cpu().numpy(), bbox=self.bbox,
                     grid_shape=np.array(self.grid_shape, dtype=np.int32))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if sorted(z.files) != sorted(cls.KEYS):
                raise ValueError("%s: expected the arrays %s, found %s"
                                 % (path, ", ".join(cls.KEYS), ", ".join(sorted(z.files))))
            return cls(z["belief"], z["bbox"], z["grid_shape"])

    # ---- the occupied voxels ---------------------------------------------------------------
    def pointcloud(self, threshold=0.5, surface_only=True):
        """-> raynet_amd.pointcloud.Pointcloud of the centres of the voxels with belief >=
        threshold, in the grid's [gx][gy][gz] order; surface_only: only those with a 6-neighbour
        below the threshold or outside the grid."""
        from .pointcloud import Pointcloud
        occ = self.belief >= float(threshold)
        keep = occ
        if surface_only:
            padded = torch.nn.functional.pad(occ, (1, 1, 1, 1, 1, 1), value=False)
            gx, gy, gz = self.grid_shape
            inner = padded[0:gx, 1:-1, 1:-1] & padded[2:gx + 2, 1:-1, 1:-1] & \
                padded[1:-1, 0:gy, 1:-1] & padded[1:-1, 2:gy + 2, 1:-1] & \
                padded[1:-1, 1:-1, 0:gz] & padded[1:-1, 1:-1, 2:gz + 2]
            keep = occ & ~inner
        centres = get_voxel_grid(self.bbox, self.grid_shape).reshape(3, -1)
        return Pointcloud(np.ascontiguousarray(centres[:, keep.reshape(-1).cpu().numpy()]))

    # ---- the surface ------------------------------------------------------------------------
    def mesh(self, threshold=0.5, closed=True):
        """-> SurfaceMesh: the surface belief = threshold, interpolated between the voxel centres
        (marching tetrahedra, HipContext.isosurface); the side belief >= threshold is inside, as
        for `pointcloud`.  closed: the grid counts as surrounded by free space, so the surface is
        closed also where the occupied region meets the border of the grid; else it is open
        there."""
        threshold = float(threshold)
        if not 0.0 < threshold <= 1.0:
            raise ValueError("threshold: a probability in (0, 1], got %r" % (threshold,))
        if not bool(torch.isfinite(self.belief).all()):
            raise ValueError("the belief has non-finite values: no surface is defined")
        ctx = self._context((1, 1), None)
        vertices, faces = ctx.isosurface(self.belief.to(ctx.device), threshold, closed)
        return SurfaceMesh(vertices, faces)

    # ---- rendering -------------------------------------------------------------------------
    def _context(self, image_shape, M):
        from .hip_implementations import get_context
        H, W = int(image_shape[0]), int(image_shape[1])
        if M is None:
            # a DDA moves monotonically along every axis: at most gx + gy + gz - 2 cells, so no
            # ray is capped (but for grids beyond the library's limit on a ray's steps)
            M = min(sum(self.grid_shape), MAX_M)
        ctx = get_context(M=int(M), H=H, W=W, bbox=self.bbox, grid_shape=self.grid_shape)
        if not ctx._grid_set:
            ctx.set_voxel_grid(np.ascontiguousarray(
                get_voxel_grid(self.bbox, self.grid_shape).transpose(1, 2, 3, 0)))
        return ctx

    def render(self, camera, image_shape, M=None):
        """The volume seen from `camera` (common.camera.Camera: P_pinv, center) at every pixel of
        an (H, W) image -> VolumeRender.  The rays are `sample_rays`' box segments; M: the cap on
        a ray's voxels (default: none that can bind)."""
        ctx = self._context(image_shape, M)
        H, W = ctx.H, ctx.W
        n = H * W
        dev = ctx.device
        ridx = torch.arange(n, dtype=torch.int32, device=dev)
        P_inv = ctx.dev(np.ascontiguousarray(camera.P_pinv, dtype=np.float32))
        center = ctx.dev(np.ascontiguousarray(camera.center, dtype=np.float32).ravel()[:3])
        starts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ends = torch.empty((n, 3), dtype=torch.float32, device=dev)
        ctx.sample_rays(ridx, P_inv, center, starts, ends)
        belief = self.belief.to(dev)
        out = torch.empty((5, n), dtype=torch.float32, device=dev)
        ctx.volume_render(starts, ends, center, belief, out)
        planes = out.cpu().numpy()
        # ray index = x * H + y: the depth maps' own orientation (forward_pass)
        return VolumeRender(*[np.ascontiguousarray(p.reshape(W, H).T) for p in planes])

    def render_scene(self, scene, frame_idxs, M=None):
        """One VolumeRender per frame of `frame_idxs`, from the scene's own cameras."""
        for i in frame_idxs:
            yield self.render(scene.get_image(i).camera, scene.image_shape, M)
