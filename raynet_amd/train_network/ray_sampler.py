"""Training batches whose rays come from many reference views, assembled on the GPU.

The reference draws one ray at a time from a Python generator -- a reference image per ray
(raynet/train_network/sample.py:495-570: `RayNetSampleGenerator`, `RayNetRandomSampleGenerator`;
sample.py:222-240: `SampleGenerator.get_sample` of the pre-training stage), rejects it when it
has no ground truth, when its ground-truth point lies outside the box or when one of its patches
crosses an image border, and fills NumPy buffers (raynet_batch_provider.py:62-95).  Here a batch
is a handful of launches:

    draw candidates (host generator) -> rn_batch_rays (points, ground-truth points, patch
    centres, rejection flags of all candidates, whatever their views) -> compact the valid ones
    -> draw again if there are too few -> voxel traversal and targets of the kept rays ->
    rn_batch_patches

`SceneBank` keeps what a scene needs on the device (images, ground-truth distance maps, camera
and neighbour tables), `RayBatchSampler` is the three generators' scene / view schedule.
"""
import collections

import numpy as np
import torch

from ..common.sampling_schemes import scheme_name
from ..hip_implementations import get_context
from .raynet_batch_provider import one_hot_target

FLAG_NAMES = ((1, "no depth"), (2, "target outside the box"), (4, "ray misses the box"),
              (8, "a patch crosses an image border"))


def camera_table(scene):
    """[V, 28] f32: P_pinv 4x3 | centre 4 | P 3x4 of every view (rn_batch_rays' `cams`)."""
    V = scene.n_images
    cams = np.zeros((V, 28), np.float32)
    for i in range(V):
        cam = scene.get_image(i).camera
        cams[i, :12] = np.asarray(cam.P_pinv, np.float32).ravel()
        cams[i, 12:16] = np.asarray(cam.center, np.float32).ravel()
        cams[i, 16:] = np.asarray(cam.P, np.float32).ravel()
    return cams


def neighbour_table(scene, neighbors):
    """[V, neighbors + 1] i32: row v = v, then v's neighbours in the scene's order."""
    return np.array([scene.view_indices_with_neighbors(i, neighbors)
                     for i in range(scene.n_images)], np.int32)


class SceneEntry(object):
    """One scene on the device."""

    def __init__(self, scene, scene_idx, gp, device):
        self.scene, self.scene_idx = scene, scene_idx
        V = scene.n_images
        H, W = scene.image_shape
        self.H, self.W, self.V = H, W, V
        dev = device
        self.images = torch.from_numpy(np.stack(
            [np.asarray(scene.get_image(i).image, np.float32).reshape(H, W, -1)
             for i in range(V)])).to(dev).contiguous()
        self.depth = torch.from_numpy(np.stack(
            [np.asarray(scene.get_depth_map(i), np.float32) for i in range(V)])).to(dev).contiguous()
        if tuple(self.depth.shape) != (V, H, W):
            raise ValueError("depth maps %s do not match the images (%d, %d, %d)"
                             % (tuple(self.depth.shape), V, H, W))
        self.cams = torch.from_numpy(camera_table(scene)).to(dev)
        self.nbr = torch.from_numpy(neighbour_table(scene, gp.neighbors)).to(dev)
        bbox = np.asarray(scene.bbox, np.float32).ravel()
        grid = tuple(int(g) for g in np.asarray(gp.grid_shape).ravel())
        padding = gp.padding if gp.padding is not None else gp.patch_shape[0]
        self.hip = get_context(gp.max_number_of_marched_voxels, gp.depth_planes, gp.neighbors + 1,
                               32, H, W, padding, bbox, grid)
        vg = np.ascontiguousarray(scene.voxel_grid(gp.grid_shape).transpose(1, 2, 3, 0))
        self.hip.set_voxel_grid(vg)
        self.voxel_grid = self.hip.dev(vg)
        self.bbox = torch.from_numpy(bbox).to(dev)
        self.grid = torch.tensor(grid, dtype=torch.float32, device=dev)
        # where on the ray the D samples lie: generation_params.sampling_type (None: the box
        # segment, through rn_batch_rays itself)
        name = scheme_name(gp)
        self.sampling_scheme = name
        self.sampling = None if name == "sample_in_bbox" else \
            self.hip.sampling(name, getattr(gp, "depth_range", None), far_from_table=True)


class SceneBank(object):
    """SceneEntry per scene index, built on first use, the `max_scenes` most recently used kept."""

    def __init__(self, dataset, generation_params, max_scenes=3, device=None):
        self.dataset, self.gp, self.max_scenes = dataset, generation_params, int(max_scenes)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self._entries = collections.OrderedDict()

    def get(self, scene_idx):
        e = self._entries.get(scene_idx)
        if e is None:
            e = SceneEntry(self.dataset.get_scene(scene_idx), scene_idx, self.gp, self.device)
            self._entries[scene_idx] = e
            while len(self._entries) > self.max_scenes:
                self._entries.popitem(last=False)
        else:
            self._entries.move_to_end(scene_idx)
        return e


class RayBatch(object):
    """inputs: the reference's list in get_batch_of_rays' layout -- N patch tensors
    [n, D, C, h, w] (channels-last memory behind that shape), voxel_grid, ray_voxel_indices,
    ray_voxel_count, S_target, points, camera_centers [n, 4] (per ray)."""

    def __init__(self, inputs, scene_idx, views, ray_idxs, targets, centres, flags, entry):
        self.inputs, self.scene_idx, self.views, self.ray_idxs = inputs, scene_idx, views, ray_idxs
        self.targets, self.centres, self.flags, self.entry = targets, centres, flags, entry

    def __len__(self):
        return int(self.ray_idxs.shape[0])


class NoValidRays(RuntimeError):
    pass


def _flag_counts(flags):
    f = flags.cpu().numpy()
    return ", ".join("%s: %d" % (name, int(((f & bit) != 0).sum())) for bit, name in FLAG_NAMES)


def evaluate_rays(entry, view, ray_idxs, patch_shape):
    """rn_batch_rays on candidates (view, ray_idxs: int32 CUDA tensors) of one scene:
    (points, target, centres, flags)."""
    hip, n = entry.hip, int(ray_idxs.shape[0])
    dev = ray_idxs.device
    N = int(entry.nbr.shape[1])
    depth = entry.depth[view.long(), (ray_idxs % entry.H).long(), (ray_idxs // entry.H).long()]
    points = torch.empty((n, hip.D, 4), dtype=torch.float32, device=dev)
    target = torch.empty((n, 4), dtype=torch.float32, device=dev)
    centres = torch.empty((n, N, hip.D, 2), dtype=torch.int32, device=dev)
    flags = torch.empty((n,), dtype=torch.int32, device=dev)
    if n:
        hip.batch_rays(view, ray_idxs, depth.contiguous(), entry.cams, entry.nbr, patch_shape,
                       points, target, centres, flags, sampling=getattr(entry, "sampling", None))
    return points, target, centres, flags


def finish_batch(entry, view, ray_idxs, points, target, centres, flags, patch_shape):
    """Traversal, voxel-space target and patches of the rays given (all of them are kept)."""
    hip, n = entry.hip, int(ray_idxs.shape[0])
    dev = ray_idxs.device
    M, D, N = hip.M, hip.D, int(entry.nbr.shape[1])
    h, w = int(patch_shape[0]), int(patch_shape[1])
    C = int(entry.images.shape[3])
    rvi = torch.zeros((n, M, 3), dtype=torch.int32, device=dev)
    rvc = torch.zeros((n,), dtype=torch.int32, device=dev)
    hip.voxel_traversal(points[:, 0, :3].contiguous(), points[:, -1, :3].contiguous(), rvi, rvc)
    voxel = torch.floor((target[:, :3] - entry.bbox[:3]) /
                        ((entry.bbox[3:] - entry.bbox[:3]) / entry.grid)).clamp_min(0).minimum(entry.grid - 1)
    S_target = one_hot_target(voxel, rvi, rvc) if n else torch.zeros((0, M), device=dev)
    patches = torch.empty((N, n, D, h, w, C), dtype=torch.float32, device=dev)
    if n:
        hip.batch_patches(entry.images, view, centres, entry.nbr, patch_shape, patches)
    # logical [n, D, C, h, w] over channels-last memory: SimpleCNN.forward_patches' first step
    # (permute to [B, h, w, C]) is then a view of contiguous memory, no copy
    per_view = [patches[j].permute(0, 1, 4, 2, 3) for j in range(N)]
    centers = entry.cams[view.long(), 12:16].contiguous()
    inputs = per_view + [entry.voxel_grid, rvi, rvc, S_target, points, centers]
    return RayBatch(inputs, entry.scene_idx, view, ray_idxs, target, centres, flags, entry)


def assemble(entry, view, ray_idxs, patch_shape, reject=True):
    """The batch of the given candidates: the valid ones in order (reject) or all of them."""
    points, target, centres, flags = evaluate_rays(entry, view, ray_idxs, patch_shape)
    if reject:
        keep = torch.nonzero(flags == 0).squeeze(1)
        view, ray_idxs, points, target, centres, flags = (
            t.index_select(0, keep).contiguous() for t in (view, ray_idxs, points, target, centres, flags))
    return finish_batch(entry, view, ray_idxs, points, target, centres, flags, patch_shape)


class RayBatchSampler(object):
    """mode "random" (RayNetRandomSampleGenerator), "window" (RayNetSampleGenerator) or
    "pretrain" (SampleGenerator.get_sample).  A batch comes from ONE scene; the generators'
    counters (rays per scene / per window position) advance once per batch, by its size.
    Everything random comes from one numpy Generator seeded with `seed`."""

    MODES = ("random", "window", "pretrain")

    def __init__(self, bank, batch_size, mode="random", scenes_range=None, n_rays=10000, window=4,
                 repeat_from_same_scene=1000, seed=0, patch_shape=None, max_rounds=8):
        if mode not in self.MODES:
            raise ValueError("mode: one of %s, got %r" % (self.MODES, mode))
        self.bank, self.batch_size, self.mode = bank, int(batch_size), mode
        self.sampling_scheme = scheme_name(bank.gp)
        if mode != "pretrain" and self.sampling_scheme != "sample_in_bbox":
            # the end-to-end batches go through the voxel traversal of the box segment and the
            # planes -> voxels mapping of evenly spaced planes on it
            raise NotImplementedError(
                "%s: the end-to-end (voxel-space) batches are sample_in_bbox only; the other "
                "schemes serve mode 'pretrain'" % self.sampling_scheme)
        n_scenes = bank.dataset.n_scenes
        self.scenes_range = list(range(n_scenes)) if scenes_range is None else list(scenes_range)
        if not self.scenes_range:
            raise ValueError("no scenes to sample from")
        self.n_rays, self.window = int(n_rays), int(window)
        self.repeat_from_same_scene = int(repeat_from_same_scene)
        self.patch_shape = tuple(bank.gp.patch_shape[:2]) if patch_shape is None else tuple(patch_shape[:2])
        self.max_rounds = int(max_rounds)
        self.rng = np.random.default_rng(seed)
        self._scene_pos, self._start, self._count = 0, 2, 0
        self._acceptance = 0.5
        self.last_start = None

    # ---- the generators' schedules -------------------------------------------------
    def _view_range(self, V):
        """[lo, hi) of the reference views of the next batch."""
        if self.mode == "random":
            lo, hi = 2, V - self.window
        elif self.mode == "window":
            lo, hi = self._start, self._start + self.window
        else:
            lo, hi = 2, V
        if not (0 <= lo < hi <= V):
            raise ValueError("a scene of %d views has no reference view in [%d, %d) (mode %r, "
                             "window %d)" % (V, lo, hi, self.mode, self.window))
        return lo, hi

    def _advance(self, V, n):
        self._count += n
        if self.mode == "random":
            if self._count >= self.n_rays:
                self._count = 0
                self._scene_pos = int(self.rng.integers(len(self.scenes_range)))
        elif self.mode == "window":
            if self._count >= self.n_rays:
                self._count = 0
                self._start += 2
                if self._start >= V - self.window:
                    self._start = 2
                    self._scene_pos = (self._scene_pos + 1) % len(self.scenes_range)
        elif self._count > self.repeat_from_same_scene:
            self._count = 0
            self._scene_pos = int(self.rng.integers(len(self.scenes_range)))

    def _draw(self, entry, lo, hi, m):
        dev = entry.cams.device
        if self.mode == "window":
            view = lo + np.floor(self.rng.random(m) * (hi - lo)).astype(np.int32)
        else:
            view = self.rng.integers(lo, hi, m).astype(np.int32)
        ridx = self.rng.integers(0, entry.H * entry.W, m).astype(np.int32)
        both = torch.from_numpy(np.stack([view, ridx])).to(dev)
        return both[0].contiguous(), both[1].contiguous()

    # ---- a batch -------------------------------------------------------------------
    def next_batch(self):
        entry = self.bank.get(self.scenes_range[self._scene_pos])
        lo, hi = self._view_range(entry.V)
        self.last_start = lo
        kept, have, seen = [], 0, []
        for _ in range(self.max_rounds):
            need = self.batch_size - have
            m = int(np.ceil(need / max(self._acceptance, 0.02) * 1.25)) + 32
            view, ridx = self._draw(entry, lo, hi, m)
            points, target, centres, flags = evaluate_rays(entry, view, ridx, self.patch_shape)
            keep = torch.nonzero(flags == 0).squeeze(1)[:need]      # (the host learns the count here)
            seen.append(flags)
            got = int(keep.shape[0])
            all_flags = torch.cat(seen)
            self._acceptance = float((all_flags == 0).float().mean())
            if got:
                kept.append(tuple(t.index_select(0, keep) for t in
                                  (view, ridx, points, target, centres, flags)))
                have += got
            if have >= self.batch_size:
                break
        if have < self.batch_size:
            raise NoValidRays("scene %d: %d valid rays of the %d asked for after %d rounds and %d "
                              "candidates (%s)" % (entry.scene_idx, have, self.batch_size,
                                                   self.max_rounds, int(all_flags.shape[0]),
                                                   _flag_counts(all_flags)))
        cols = [torch.cat(c).contiguous() if len(kept) > 1 else c[0].contiguous() for c in zip(*kept)]
        batch = finish_batch(entry, *cols, patch_shape=self.patch_shape)
        self._advance(entry.V, self.batch_size)
        return batch

    def __iter__(self):
        while True:
            yield self.next_batch()
