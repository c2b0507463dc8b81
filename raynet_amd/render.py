"""A surface mesh seen from cameras: the finished surface turned back into images.

`render_mesh` casts one ray per pixel of every camera through the mesh's BVH, all views in one
launch (include/raynet_hip.h, rn_mesh_render; csrc/raynet_render.inl), and
returns per pixel the face the ray hits first, the depth of the hit -- the bits
`MeshRaycaster.depth_map` gives --, where in the face it lies (the Moeller-Trumbore u, v) and the
vertices' colours and normals interpolated there.  Face and barycentrics are what every later
image-space consumer needs: textures, per-face visibility, any per-vertex quantity as an image.

`MeshRender` turns the planes into 8-bit images; `metrics.photometric_error` scores a colour
render against the photograph it was coloured from.

There is no CPU route: without a GPU the ray caster raises RaynetHipError.
"""
import numpy as np
import torch


def camera_rows(cameras):
    """(V, 15) float32: per camera P_pinv [4][3] row-major | centre [3], what rn_mesh_render and
    rn_mesh_depthmap read."""
    rows = [np.concatenate([np.asarray(c.P_pinv, np.float32).reshape(12),
                            np.asarray(c.center, np.float32).reshape(-1)[:3]]) for c in cameras]
    return np.stack(rows).astype(np.float32) if rows else np.zeros((0, 15), np.float32)


def _rgb8(planes):
    """(H, W, C) float in [0, 1] -> (H, W, 3) uint8 (appearance.to_rgb8's rule)."""
    from .appearance import to_rgb8
    H, W = planes.shape[:2]
    return to_rgb8(planes.reshape(H * W, -1)).reshape(H, W, 3)


class MeshRender(object):
    """What `render_mesh` returns, device tensors over (V, H, W): face int32 (-1: the ray hits
    nothing), depth float32 (0 there), bary (.., 2) float32, color (.., C) float32 or None, normal
    (.., 3) float32 or None, and mask = face >= 0."""
    __slots__ = ("face", "depth", "bary", "color", "normal", "mask")

    def __init__(self, face, depth, bary, color, normal):
        self.face, self.depth, self.bary, self.color, self.normal = face, depth, bary, color, normal
        self.mask = face >= 0

    def rgb8(self, view, background=(0, 0, 0)):
        """(H, W, 3) uint8: the colour image of one view, rint(clip(c, 0, 1) * 255), `background`
        (8-bit values) where the ray hits nothing.  One channel gives grey."""
        if self.color is None:
            raise ValueError("the mesh was rendered without colours")
        out = _rgb8(self.color[view].cpu().numpy())
        out[~self.mask[view].cpu().numpy()] = np.asarray(background, np.uint8)
        return out

    def normal_rgb8(self, view):
        """(H, W, 3) uint8: (n + 1) / 2 as an image, black where the ray hits nothing."""
        if self.normal is None:
            raise ValueError("the mesh was rendered without normals")
        out = _rgb8((self.normal[view].cpu().numpy() + np.float32(1)) / np.float32(2))
        out[~self.mask[view].cpu().numpy()] = 0
        return out

    def shaded8(self, view, cameras):
        """(H, W, 3) uint8: a grey headlight image max(0, n . unit(c - p)) of one view, for meshes
        without colours; p is the hit (the pixel's ray at the rendered depth), c the camera's
        centre.  Torch operations on the outputs: a convenience, not to the bit."""
        if self.normal is None:
            raise ValueError("the mesh was rendered without normals")
        from .mesh import pixel_destinations
        cam = cameras[view]
        H, W = self.depth.shape[1:]
        ys, xs = np.mgrid[0:H, 0:W]
        centre = np.asarray(cam.center, np.float32).reshape(-1)[:3]
        towards = pixel_destinations(cam.P_pinv, xs.reshape(-1), ys.reshape(-1)) - centre
        to_camera = torch.from_numpy(-towards).to(self.normal.device).reshape(H, W, 3)
        to_camera = to_camera / to_camera.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        grey = (self.normal[view] * to_camera).sum(-1).clamp(0, 1) * self.mask[view]
        return _rgb8(grey.cpu().numpy()[:, :, None])

    def textured(self, texture, bilinear=True):
        """-> a MeshRender with the same planes whose colour is `texture` (texture.MeshTexture of
        the rendered mesh's faces) looked up at every pixel's face and barycentrics, bilinear or
        the nearest texel (texture.sample_texture)."""
        from .texture import sample_texture
        return MeshRender(self.face, self.depth, self.bary,
                          sample_texture(self, texture, bilinear), self.normal)


def render_mesh(mesh, cameras, H, W, raycaster=None):
    """-> MeshRender of `mesh` (volume.SurfaceMesh; its uint8 colours go in as /255 float32) seen
    by `cameras` (common.camera.Camera objects) at H x W pixels.  raycaster: mesh.raycaster(), to
    build the BVH once for several calls.  An empty mesh raises ValueError."""
    if mesh.empty:
        raise ValueError("the mesh is empty: there is no surface to render")
    caster = mesh.raycaster() if raycaster is None else raycaster
    if caster.n_triangles != len(mesh.faces):
        raise ValueError("raycaster: a BVH of %d triangles for a mesh of %d faces"
                         % (caster.n_triangles, len(mesh.faces)))
    device = caster.device

    def upload(a, dtype):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)

    colors = mesh.colors
    if colors is not None and colors.dtype == np.uint8:
        colors = colors.astype(np.float32) / np.float32(255)
    with torch.cuda.device(device):
        out = caster._ctx.mesh_render(caster.nodes, caster.leaves, upload(mesh.vertices, np.float32),
                                      upload(mesh.faces, np.int32),
                                      upload(camera_rows(cameras), np.float32), H, W,
                                      upload(colors, np.float32), upload(mesh.normals, np.float32))
    return MeshRender(*out)
