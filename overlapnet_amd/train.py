"""Fitting the overlap (Delta) head on frozen legs: the reference's `360OutputkLegsFixed` training (src/two_heads/training.py) cut
down to the one part of the network that is both geometry-dependent and trainable once the legs are frozen.

The gradients come from the HIP library (`OvnEngine.delta_head_grad`, csrc/delta_head_backward.hip); the optimizer is the
reference's Adagrad (training.py:253) as elementwise torch on the device -- plumbing, not a kernel.  Leg gradients and the yaw
loss (it has no parameter downstream of frozen legs) are out of scope.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import weights as W
from ._lib import OvnError


def lr_schedule(epoch: int, initial_lr: float, alpha: float) -> float:
    """The reference's learning-rate schedule (training.py:47-57): a tenth of the rate in epoch 0, then lr alpha^(epoch - 1)."""
    if epoch == 0:
        return initial_lr * 0.1
    return initial_lr * np.power(alpha, epoch - 1.0)


def adagrad_step(params: Sequence[torch.Tensor], accum: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], lr: float,
                 eps: float = 1e-7) -> None:
    """Keras 2.1.5's Adagrad, in place: a += g^2; p -= lr g / (sqrt(a) + eps)."""
    for p, a, g in zip(params, accum, grads):
        a.add_(g * g)
        p.sub_(lr * g / (torch.sqrt(a) + eps))


def epoch_batches(n: int, batch_size: int, epoch: int, seed: int = 0) -> List[np.ndarray]:
    """Shuffled mini-batches of the pair positions 0 .. n - 1 for one epoch; the last, partial batch is kept (as the reference's
    Sequence does).  The order depends on (seed, epoch) alone."""
    perm = np.random.default_rng([int(seed), int(epoch)]).permutation(int(n))
    bs = max(1, int(batch_size))
    return [perm[a:a + bs] for a in range(0, int(n), bs)]


class OverlapHeadTrainer(object):
    """Adagrad on the eight Delta-head tensors of `infer`'s engine, over pairs of `infer.feature_volumes`.

    loss: 'sigmoid' (the reference's my_sigmoid_loss) or 'mse'; loss_weight: the reference's lossWeights['overlap_output'], the
    `scale` of the gradient call.  Every step re-registers the head, so the `infer_*` calls use the new head at once; when `step` /
    `fit` return, the Delta cache rows of `infer.feature_volumes` have been rebuilt under it and the look-ahead context (which holds
    a head of its own) has been dropped."""

    def __init__(self, infer, learning_rate: float, lr_alpha: float = 0.99, loss: str = "sigmoid", loss_weight: float = 5.0):
        if getattr(infer, "_world", 1) > 1:
            raise OvnError("OverlapHeadTrainer: not available on a sharded Infer (world %d)" % infer._world)
        self.infer = infer
        self.engine = infer.engine
        self.learning_rate, self.lr_alpha = float(learning_rate), float(lr_alpha)
        self.loss, self.loss_weight = loss, float(loss_weight)
        if loss not in self.engine._LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(self.engine._LOSSES), loss))
        self.epoch = 0
        self.last: Optional[dict] = None      # result of the most recent gradient call (its overlaps are those BEFORE the update)
        dev = self.engine.device
        self.params: List[torch.Tensor] = []
        for name in self.engine.HEAD_PARAMS:
            k = np.ascontiguousarray(infer._weights[name], np.float32)
            if name == "c_conv1/kernel" and self.engine.negate_diffs:
                k = -k                          # as registered (engine.load_weights)
            self.params.append(torch.from_numpy(k).to(dev))
        self.accum = [torch.zeros_like(p) for p in self.params]

    # -- one update ---------------------------------------------------------------------------------
    def _grad(self, left_idx, right_idx, overlaps):
        feats = self.infer.feature_volumes.device_features
        r = self.engine.delta_head_grad(feats, feats, overlaps, lidx=left_idx, ridx=right_idx, loss=self.loss, scale=self.loss_weight)
        return r, [r["grads"][n.split("/")[0]][n.split("/")[1]] for n in self.engine.HEAD_PARAMS]

    def gradients(self, left_idx, right_idx, overlaps) -> Dict[str, torch.Tensor]:
        """The gradients of one batch with respect to the tensors of the weight FILE, by HEAD_PARAMS name (the library differentiates
        the c_conv1 kernel it holds, which is the file's negated under deltaLayer_negateDiffs: that sign is undone here), plus
        'loss' and 'overlap'.  No update."""
        r, grads = self._grad(left_idx, right_idx, overlaps)
        out = {n: (-g if (n == "c_conv1/kernel" and self.engine.negate_diffs) else g) for n, g in zip(self.engine.HEAD_PARAMS, grads)}
        out["loss"], out["overlap"] = r["loss"], r["overlap"]
        return out

    def _update(self, left_idx, right_idx, overlaps) -> torch.Tensor:
        r, grads = self._grad(left_idx, right_idx, overlaps)
        adagrad_step(self.params, self.accum, grads, float(lr_schedule(self.epoch, self.learning_rate, self.lr_alpha)))
        self.engine.set_head_weights(self.params)
        self.last = r
        return r["loss"]

    def _head_changed(self) -> None:
        inf = self.infer
        inf._drop_ahead()
        if inf._qa is not None:                 # the look-ahead context registered the old head
            inf._qa.close()
            inf._qa = None
        inf._weights = self.weights()
        inf.feature_volumes.rebuild_delta_cache()

    def step(self, left_idx, right_idx, overlaps) -> float:
        """One Adagrad step on the pairs (feature_volumes[left_idx[p]] -> head-left, [right_idx[p]] -> head-right) with targets
        `overlaps`, at the current epoch's learning rate.  Returns the loss before the update."""
        loss = self._update(left_idx, right_idx, overlaps)
        self._head_changed()
        return float(loss)

    def fit(self, left_idx, right_idx, overlaps, epochs: int, batch_size: Optional[int] = None, seed: int = 0) -> List[float]:
        """`epochs` passes over the pairs in shuffled mini-batches (`epoch_batches`; batch_size defaults to infer.batch_size).
        Returns the loss of every step."""
        li = np.asarray(left_idx, np.int64).reshape(-1)
        ri = np.asarray(right_idx, np.int64).reshape(-1)
        ov = np.asarray(overlaps, np.float32).reshape(-1)
        if not (len(li) == len(ri) == len(ov)) or len(li) == 0:
            raise ValueError("fit: %d left, %d right indices and %d overlaps" % (len(li), len(ri), len(ov)))
        bs = int(self.infer.batch_size if batch_size is None else batch_size)
        losses = []
        try:
            for _ in range(int(epochs)):
                for b in epoch_batches(len(li), bs, self.epoch, seed):
                    losses.append(self._update(li[b], ri[b], ov[b]))
                self.epoch += 1
        finally:
            self._head_changed()
        return [float(v) for v in torch.cat(losses).cpu()] if losses else []

    def fit_from_npz(self, npz_files: Sequence[str], epochs: int, batch_size: Optional[int] = None, seed: int = 0,
                     no_pairs: Optional[int] = None) -> List[float]:
        """`fit` on the pairs of the reference's ground-truth npz files (evaluate.load_pairs) with the roles of evaluate.run_test:
        imgf1 -> head-left, imgf2 -> head-right.  The scans that occur are run through the leg into `infer.feature_volumes`."""
        from .evaluate import load_pairs
        from .infer import FeatureVolumeCache
        f1, f2, _d1, _d2, ov, _yaw = load_pairs(npz_files, shuffle=False)
        n = len(f1) if no_pairs is None else min(int(no_pairs), len(f1))
        if n == 0:
            raise Exception("no training pairs")
        f1, f2, ov = f1[:n], f2[:n], ov[:n]
        names = sorted(set(f1) | set(f2))
        pos = {name: i for i, name in enumerate(names)}
        cache = FeatureVolumeCache(self.engine, min_capacity=len(names))
        cache.extend_device(self.infer._leg_device(names))
        self.infer.feature_volumes = cache
        return self.fit([pos[v] for v in f1], [pos[v] for v in f2], ov, epochs, batch_size, seed)

    # -- results ------------------------------------------------------------------------------------
    def weights(self) -> Dict[str, np.ndarray]:
        """The full weight dict by Keras layer name: the legs untouched, the head as fitted (negateDiffs undone: the file's kernel)."""
        out = dict(self.infer._weights)
        for name, p, shape in zip(self.engine.HEAD_PARAMS, self.params, self.engine.head_param_shapes()):
            a = p.detach().cpu().numpy().reshape(shape).copy()
            out[name] = -a if (name == "c_conv1/kernel" and self.engine.negate_diffs) else a
        return out

    def save(self, path: str) -> None:
        """Write `weights()` as npz; the file loads through config['pretrained_weightsfilename']."""
        W.save_npz(path, self.weights())
