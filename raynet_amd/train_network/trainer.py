"""The two training loops: pre-training of the MV-CNN on depth-space targets
(raynet/scripts/pretrain_network.py, Keras `fit_generator`) and the end-to-end training through
the MRF block (raynet/scripts/train_raynet.py:263-301 around
tf_implementations/forward_backward_pass.py `build_end_to_end_training`).

Both draw their batches from a `RayBatchSampler`, write `train_statistics.txt`
(`scene_idx max_img_idx loss gamma`, one line per step) and `val_loss.txt` (one line per
validation on a fixed set drawn once), and save `weights.%d.npz` -- the reference's 30 arrays in
its order, what `scripts/forward_pass.py --weight_file` loads -- next to `state.%d.pt` (model
buffers, optimiser, gamma, step, sampler state) for `--resume`.

Batch normalisation: the reference builds its end-to-end graph under `K.set_learning_phase(0)`
(forward_backward_pass.py:2), i.e. the CNN runs with its moving statistics while its weights
train; `batch_norm="frozen"` (`model.eval()`, gradients still flow) is therefore the end-to-end
default, `"batch"` uses batch statistics in the steps.  Pre-training uses batch statistics and
validates in inference mode, as `fit_generator` does.
"""
import glob
import os
import re

import numpy as np
import torch

from .. import loss_functions
from ..hip_implementations.forward_backward_pass import (depth_distribution_from_features,
                                                         forward_backward_pass)

STATISTICS_HEADER = "scene_idx max_img_idx loss gamma"


def make_optimizer(params, name="Adam", lr=1e-3, momentum=0.9):
    """--optimizer / --lr / --momentum as the reference's models.py hands them to Keras."""
    if name == "Adam":
        return torch.optim.Adam(params, lr=lr, eps=1e-7)        # (Keras' epsilon)
    if name == "SGD":
        return torch.optim.SGD(params, lr=lr, momentum=momentum)
    raise ValueError("optimizer: Adam or SGD, got %r" % (name,))


def l2_penalty(model, weight_decay):
    """Keras `kernel_regularizer=l2(weight_decay)` on the convolution kernels: added to the loss."""
    if not weight_decay:
        return 0.0
    return weight_decay * sum((m.weight ** 2).sum() for m in model.modules()
                              if isinstance(m, torch.nn.Conv2d))


def clip_per_tensor(params, clipnorm):
    """Keras `clipnorm`: every gradient tensor is scaled down to norm `clipnorm` on its own."""
    for p in params:
        if p.grad is not None:
            norm = p.grad.norm()
            p.grad.mul_(torch.clamp(clipnorm / (norm + 1e-12), max=1.0))


def pretrain_loss(model, batch, views, target_distribution_factory, loss):
    """MV-CNN on the patches -> softmax over the D hypotheses -> loss against the depth-space
    target distribution of the rays' ground-truth points."""
    patches, points = batch.inputs[:views], batch.inputs[views + 4]
    n, D = patches[0].shape[:2]
    features = [model(p.reshape((n * D,) + tuple(p.shape[2:]))).reshape(n, D, -1) for p in patches]
    S = depth_distribution_from_features(features, views)
    y = target_distribution_factory(batch.targets, points)
    return loss_functions.loss_factory(loss)(y, S).mean()


def raynet_loss(model, batch, views, gamma, bp_iterations, loss):
    patches = batch.inputs[:views]
    voxel_grid, rvi, rvc, S_target, points, centers = batch.inputs[views:]
    return forward_backward_pass(model, patches, voxel_grid, rvi, rvc, S_target, points, centers,
                                 batch.entry.hip, views=views, gamma=gamma,
                                 bp_iterations=bp_iterations, loss=loss)


def draw_validation_set(sampler, n_samples):
    """A fixed list of batches holding n_samples rays (the last batch is cut)."""
    batches, have = [], 0
    while have < n_samples:
        b = sampler.next_batch()
        batches.append(b)
        have += len(b)
    return batches


class Trainer(object):
    """stage "raynet" (end to end, forward_backward_pass) or "pretrain" (depth-space targets)."""

    def __init__(self, model, stage, views, output_directory, loss="emd", optimizer="Adam", lr=1e-3,
                 momentum=0.9, weight_decay=0.0, clipnorm=None, batch_norm=None, gamma=0.031,
                 gamma_range=(1e-3, 0.99), train_with_gamma=False, bp_iterations=3,
                 target_distribution_factory=None):
        assert stage in ("raynet", "pretrain")
        self.model, self.stage, self.views = model, stage, int(views)
        self.output_directory = output_directory
        self.loss, self.weight_decay, self.clipnorm = loss, weight_decay, clipnorm
        self.batch_norm = batch_norm or ("frozen" if stage == "raynet" else "batch")
        assert self.batch_norm in ("frozen", "batch")
        self.bp_iterations = bp_iterations
        self.target_distribution_factory = target_distribution_factory
        if stage == "pretrain" and target_distribution_factory is None:
            raise ValueError("pre-training needs a target_distribution_factory")
        dev = next(model.parameters()).device
        self.gamma = torch.tensor(float(gamma), device=dev,
                                  requires_grad=bool(train_with_gamma) and stage == "raynet")
        self.gamma_range = (float(gamma_range[0]), float(gamma_range[1]))
        self.params = list(model.parameters()) + ([self.gamma] if self.gamma.requires_grad else [])
        self.optimizer = make_optimizer(self.params, optimizer, lr, momentum)
        self.step, self.snapshots = 0, 0
        # the batches are patches: the row-matrix path whatever their number (models.py)
        model.patch_path = True

    # ---- one step / one validation --------------------------------------------------
    def _loss(self, batch):
        if self.stage == "pretrain":
            return pretrain_loss(self.model, batch, self.views, self.target_distribution_factory,
                                 self.loss)
        return raynet_loss(self.model, batch, self.views, self.gamma, self.bp_iterations, self.loss)

    def train_step(self, batch):
        self.model.train(self.batch_norm == "batch")
        self.optimizer.zero_grad()
        loss = self._loss(batch)
        (loss + l2_penalty(self.model, self.weight_decay)).backward()
        if self.clipnorm:
            clip_per_tensor(self.params, self.clipnorm)
        self.optimizer.step()
        if self.gamma.requires_grad:
            with torch.no_grad():
                self.gamma.clamp_(*self.gamma_range)
        return float(loss.detach())

    pretrain_step = train_step

    @torch.no_grad()
    def validate(self, batches):
        self.model.eval()
        total = sum(float(self._loss(b)) * len(b) for b in batches)
        return total / sum(len(b) for b in batches)

    # ---- snapshots ------------------------------------------------------------------
    def snapshot(self, sampler=None, lines=None):
        out = self.output_directory
        np.savez(os.path.join(out, "weights.%d.npz" % self.snapshots), *self.model.reference_weights())
        state = {"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(),
                 "gamma": float(self.gamma.detach()), "step": self.step,
                 "snapshots": self.snapshots + 1, "lines": lines,
                 "sampler": None if sampler is None else sampler_state(sampler)}
        torch.save(state, os.path.join(out, "state.%d.pt" % self.snapshots))
        self.snapshots += 1

    def resume(self, sampler=None):
        """Load the newest state.%d.pt of the output directory; returns its `lines` (statistics
        lines written when it was saved) or None when there is nothing to resume from."""
        files = glob.glob(os.path.join(self.output_directory, "state.*.pt"))
        if not files:
            return None
        newest = max(files, key=lambda f: int(re.search(r"state\.(\d+)\.pt$", f).group(1)))
        state = torch.load(newest, map_location=self.gamma.device, weights_only=False)
        self.model.load_state_dict(state["model"])
        self.optimizer.load_state_dict(state["optimizer"])
        with torch.no_grad():
            self.gamma.fill_(state["gamma"])
        self.step, self.snapshots = state["step"], state["snapshots"]
        if sampler is not None and state["sampler"] is not None:
            restore_sampler(sampler, state["sampler"])
        return state["lines"] or (0, 0)

    # ---- the loop -------------------------------------------------------------------
    def fit(self, sampler, validation, iterations, validate_every, snapshot_every, resume=False,
            log=None):
        """train_raynet.py:263-301: a step, its statistics line, every `validate_every` steps a
        validation line, every `snapshot_every` steps a snapshot -- and one at the end, so that
        the trained weights are always on disk."""
        out = self.output_directory
        os.makedirs(out, exist_ok=True)
        train_path = os.path.join(out, "train_statistics.txt")
        val_path = os.path.join(out, "val_loss.txt")
        lines = self.resume(sampler) if resume else None
        if lines is None:
            with open(train_path, "w") as f:
                f.write(STATISTICS_HEADER + "\n")
            open(val_path, "w").close()
            lines = (0, 0)
        else:       # what a run wrote past its last snapshot is written again by this one
            _truncate(train_path, 1 + lines[0])
            _truncate(val_path, lines[1])
        n_train, n_val = lines
        with open(train_path, "a") as train_f, open(val_path, "a") as val_f:
            while self.step < iterations:
                it = self.step
                batch = sampler.next_batch()
                loss = self.train_step(batch)
                train_f.write("%d %d %s %s\n" % (batch.scene_idx, int(batch.views.max()), repr(loss),
                                                 repr(float(self.gamma.detach()))))
                train_f.flush()
                n_train += 1
                if it % validate_every == 0:
                    val = self.validate(validation)
                    val_f.write(repr(val) + "\n")
                    val_f.flush()
                    n_val += 1
                    if log:
                        log("validation loss in iteration %d: %f - gamma: %f"
                            % (it, val, float(self.gamma.detach())))
                self.step = it + 1
                if it % snapshot_every == 0 or self.step == iterations:
                    self.snapshot(sampler, (n_train, n_val))
        return self


def _truncate(path, n_lines):
    with open(path) as f:
        kept = f.readlines()[:n_lines]
    with open(path, "w") as f:
        f.writelines(kept)


def sampler_state(s):
    return {"rng": s.rng.bit_generator.state, "scene_pos": s._scene_pos, "start": s._start,
            "count": s._count, "acceptance": s._acceptance}


def restore_sampler(s, state):
    s.rng.bit_generator.state = state["rng"]
    s._scene_pos, s._start, s._count = state["scene_pos"], state["start"], state["count"]
    s._acceptance = state["acceptance"]
