"""Fitting the overlap (Delta) head on frozen legs: the reference's `360OutputkLegsFixed` training (src/two_heads/training.py) cut
down to the one part of the network that is both geometry-dependent and trainable once the legs are frozen.

The gradients come from the HIP library (`OvnEngine.delta_head_grad`, csrc/delta_head_backward.hip); the optimizer is the
reference's Adagrad (training.py:253) as elementwise torch on the device -- plumbing, not a kernel.

Training the legs: the yaw head has no weights, so the reference's orientation loss (`my_entropy`, training.py:86-92) acts only
through the leg outputs, and `OverlapHeadTrainer` (frozen legs) has no use for it.  `heads_loss` is where it exists: both heads'
losses as ONE differentiable scalar of the feature-volume pools (`OvnEngine.heads_feature_grad`, csrc/heads_feature_grad.hip: the
overlap loss and the yaw loss differentiated down to the leg outputs on the GPU).  A leg written in torch plugs into it and gets
d L / d (its output) from `backward()`.

Training the whole network: `OverlapNetTrainer` is the reference's default training step (training.py: both losses, all tensors of
the Siamese network, Adagrad).  The leg's forward with stored activations and its backward run in the library
(`OvnEngine.leg_forward_train` / `leg_backward`, csrc/leg_backward.hip); the chain is leg forward -> `heads_feature_grad` ->
`sum_rows_by_entry` for both sides (the leg is shared: a scan that is left in one pair and right in another gets both sums) ->
leg backward -> Adagrad on the 8 head and 2 x layers leg tensors.

Training on every GPU of a node: `DataParallelTrainer` runs that chain on each rank's share of the global batch; the ranks' flat
gradients meet in one all-gather (`distributed.exchange_gradients`), and the share-weighted sum in a fixed order plus Adagrad on one
flat parameter buffer is a kernel (`OvnEngine.grad_reduce_adagrad`, csrc/grad_reduce.hip): behind a collective the update is on the
critical path of every rank.
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


def sum_rows_by_entry(rows: torch.Tensor, idx, entries: int) -> torch.Tensor:
    """rows (n, ...) -> (entries, ...): out[e] = the sum of rows[p] over the pairs p with idx[p] == e, in a fixed order, so the
    same bits every time: the pairs are sorted by entry (stable: pair order inside an entry) and every entry's run is summed by one
    pairwise tree -- round d adds, inside each run, position r + d onto position r for the r that are multiples of 2 d.  Within a
    round no destination occurs twice, so no float `index_add_` and no atomics; ceil(log2(longest run)) rounds, each one indexed
    add over the rows, whatever the batch size (the 1-vs-N form, in which every pair addresses entry 0, costs log2 N rounds).  An
    index list that lives on the device is copied to the host once."""
    idx = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, np.int64).reshape(-1)
    if len(idx) != rows.shape[0]:
        raise ValueError("%d indices for %d rows" % (len(idx), rows.shape[0]))
    out = torch.zeros((int(entries),) + tuple(rows.shape[1:]), dtype=rows.dtype, device=rows.device)
    if len(idx) == 0:
        return out
    order = np.argsort(idx, kind="stable")
    si = idx[order]
    start = np.concatenate([[0], np.flatnonzero(si[1:] != si[:-1]) + 1])
    length = np.diff(np.concatenate([start, [len(si)]]))
    rank = np.arange(len(si)) - np.repeat(start, length)
    left = np.repeat(length, length) - rank                      # rows from this position to the end of its run
    buf = rows[torch.from_numpy(order).to(rows.device)]
    d = 1
    while d < int(length.max()):
        dst = torch.from_numpy(np.flatnonzero((rank % (2 * d) == 0) & (left > d))).to(rows.device)
        buf[dst] = buf[dst] + buf[dst + d]
        d *= 2
    out[torch.from_numpy(si[start]).to(rows.device)] = buf[torch.from_numpy(start).to(rows.device)]
    return out


class _HeadsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats_l, feats_r, engine, targets, yaw_bins, lidx, ridx, kw):
        fl, fr = feats_l.detach().contiguous(), feats_r.detach().contiguous()
        r = engine.heads_feature_grad(fl, fr, targets, yaw_bins, lidx=lidx, ridx=ridx, want_corr=False, **kw)    # the one engine call
        n = r["overlap"].numel()
        nl, nr = fl.numel() // (engine._fw * 128), fr.numel() // (engine._fw * 128)
        # a pool that asks for no gradient (a frozen leg, torch.no_grad()) gets no sum and keeps nothing
        ctx.gl = ctx.gr = None
        if ctx.needs_input_grad[0]:
            ctx.gl = sum_rows_by_entry(r["dfeat_l"], np.arange(n) if lidx is None else lidx, nl).view(feats_l.shape)
        if ctx.needs_input_grad[1]:
            ctx.gr = sum_rows_by_entry(r["dfeat_r"], np.zeros(n, np.int64) if ridx is None else ridx, nr).view(feats_r.shape)
        return r["loss_overlap"] + r["loss_yaw"]

    @staticmethod
    def backward(ctx, g):
        return (None if ctx.gl is None else g * ctx.gl, None if ctx.gr is None else g * ctx.gr, None, None, None, None, None, None)


def heads_loss(engine, feats_l: torch.Tensor, feats_r: torch.Tensor, targets, yaw_bins, lidx=None, ridx=None, loss: str = "sigmoid",
               overlap_scale: float = 5.0, yaw_scale: float = 1.0, min_overlap_for_angle: float = 0.7) -> torch.Tensor:
    """The reference's training loss of a batch of pairs, lossWeights included (training.py:240-252), as a 0-dim tensor that is
    differentiable with respect to the feature-volume pools feats_l (k, W, 128) and feats_r (the same tensor may be both):
    overlap_scale / n sum_p loss(overlap_p, targets[p]) + yaw_scale / (n W) sum of the weighted cross entropy of the correlation
    logits against yaw_bins (`OvnEngine.heads_feature_grad`; pairs as in `heads`: lidx None -> p, ridx None -> 0, the 1-vs-N form in
    which every pair addresses right entry 0).  The engine runs once, in forward; backward hands each pool the per-pair rows summed
    over the pairs that address each entry, in a fixed order (`sum_rows_by_entry`: deterministic).  The head weights are constants here;
    their gradients come from `OvnEngine.heads_feature_grad(..., want_head_grads=True)` or `delta_head_grad`."""
    kw = dict(loss=loss, overlap_scale=overlap_scale, yaw_scale=yaw_scale, min_overlap_for_angle=min_overlap_for_angle)
    return _HeadsLoss.apply(feats_l, feats_r, engine, targets, yaw_bins, lidx, ridx, kw)


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


class OverlapNetTrainer(object):
    """The reference's full training step (training.py) on `infer`'s engine: Adagrad on the eight head tensors and the 2 x layers
    leg tensors under  overlap_scale / n sum_p loss(overlap_p, t_p)  +  yaw_scale / (n W) sum of the weighted cross entropy of the
    correlation logits against the yaw bins (`OvnEngine.heads_feature_grad`).  A batch is given by scan NAMES (the cue files
    `Infer._inputs_device` reads): pair p = (left_names[p] -> head-left, right_names[p] -> head-right).

    train_legs=False keeps the legs frozen (the reference's `360OutputkLegsFixed`): the yaw loss then has nothing to act on and only
    the head tensors move.  Every step re-registers the weights it changed.  When `step` / `fit` return, the look-ahead context
    (which holds weights of its own) is closed, `infer._weights` is current, and `infer.feature_volumes` is empty: every cached
    volume, spectrum and Delta row was computed by the old legs (train_legs=False: the volumes stay, their Delta rows are rebuilt)."""

    def __init__(self, infer, learning_rate: float, lr_alpha: float = 0.99, loss: str = "sigmoid", overlap_scale: float = 5.0,
                 yaw_scale: float = 1.0, min_overlap_for_angle: float = 0.7, train_legs: bool = True):
        if getattr(infer, "_world", 1) > 1:
            raise OvnError("OverlapNetTrainer: not available on a sharded Infer (world %d)" % infer._world)
        self.infer = infer
        self.engine = infer.engine
        self.learning_rate, self.lr_alpha = float(learning_rate), float(lr_alpha)
        self.loss, self.overlap_scale, self.yaw_scale = loss, float(overlap_scale), float(yaw_scale)
        self.min_overlap_for_angle, self.train_legs = float(min_overlap_for_angle), bool(train_legs)
        if loss not in self.engine._LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(self.engine._LOSSES), loss))
        self.epoch = 0
        self.last: Optional[dict] = None      # result of the most recent heads_feature_grad call (values BEFORE the update)
        dev = self.engine.device
        self.head_names = list(self.engine.HEAD_PARAMS)
        self.leg_names = self.engine.leg_param_names()
        self.names = self.head_names + self.leg_names         # the 8 + 2 x layers tensors, in the order of `params`
        self.params: List[torch.Tensor] = []
        for name in self.names:
            k = np.ascontiguousarray(infer._weights[name], np.float32)
            if name == "c_conv1/kernel" and self.engine.negate_diffs:
                k = -k                          # as registered (engine.load_weights)
            self.params.append(torch.from_numpy(k).to(dev))
        self.accum = [torch.zeros_like(p) for p in self.params]

    # -- the chain ----------------------------------------------------------------------------------
    @staticmethod
    def _pool(left_names, right_names):
        """The unique scans of a batch (sorted) and each pair's two positions among them."""
        ln, rn = [str(v) for v in left_names], [str(v) for v in right_names]
        if len(ln) != len(rn) or not ln:
            raise ValueError("%d left and %d right names (at least one pair)" % (len(ln), len(rn)))
        names = sorted(set(ln) | set(rn))
        pos = {v: i for i, v in enumerate(names)}
        return names, np.array([pos[v] for v in ln], np.int64), np.array([pos[v] for v in rn], np.int64)

    def _chain(self, left_names, right_names, overlaps, yaw_bins):
        names, lidx, ridx = self._pool(left_names, right_names)
        x = self.infer._inputs_device(names)
        acts = self.engine.leg_forward_train(x)
        feats = acts[-1].view(len(names), self.engine.feat_w, 128)
        r = self.engine.heads_feature_grad(feats, feats, overlaps, yaw_bins, lidx=lidx, ridx=ridx, loss=self.loss,
                                           overlap_scale=self.overlap_scale, yaw_scale=self.yaw_scale,
                                           min_overlap_for_angle=self.min_overlap_for_angle, want_head_grads=True, want_corr=False)
        grads = [r["grads"][n.split("/")[0]][n.split("/")[1]] for n in self.head_names]
        if self.train_legs:
            dfeat = sum_rows_by_entry(r["dfeat_l"], lidx, len(names)) + sum_rows_by_entry(r["dfeat_r"], ridx, len(names))
            leg = self.engine.leg_backward(x, acts, dfeat)
            grads += [leg[n] for n in self.leg_names]
        return r, grads

    def gradients(self, left_names, right_names, overlaps, yaw_bins) -> Dict[str, torch.Tensor]:
        """The gradients of one batch with respect to the tensors of the weight FILE, by Keras name (the c_conv1 kernel's sign under
        deltaLayer_negateDiffs is undone, as in OverlapHeadTrainer.gradients; train_legs=False: the head tensors only), plus
        'loss_overlap', 'loss_yaw' and 'overlap'.  No update."""
        r, grads = self._chain(left_names, right_names, overlaps, yaw_bins)
        out = {n: (-g if (n == "c_conv1/kernel" and self.engine.negate_diffs) else g) for n, g in zip(self.names, grads)}
        out["loss_overlap"], out["loss_yaw"], out["overlap"] = r["loss_overlap"], r["loss_yaw"], r["overlap"]
        return out

    def _update(self, left_names, right_names, overlaps, yaw_bins) -> torch.Tensor:
        r, grads = self._chain(left_names, right_names, overlaps, yaw_bins)
        k = len(grads)
        adagrad_step(self.params[:k], self.accum[:k], [g.reshape(p.shape) for g, p in zip(grads, self.params)],
                     float(lr_schedule(self.epoch, self.learning_rate, self.lr_alpha)))
        self.engine.set_head_weights(self.params[:8])
        if self.train_legs:
            self.engine.set_leg_weights(dict(zip(self.leg_names, self.params[8:])))
        self.last = r
        return (r["loss_overlap"] + r["loss_yaw"]).reshape(1)

    def _weights_changed(self) -> None:
        inf = self.infer
        inf._drop_ahead()
        if inf._qa is not None:                 # the look-ahead context registered the old weights
            inf._qa.close()
            inf._qa = None
        inf._weights = self.weights()
        if self.train_legs:
            inf.feature_volumes = []
        else:
            inf.feature_volumes.rebuild_delta_cache()

    def step(self, left_names, right_names, overlaps, yaw_bins) -> float:
        """One Adagrad step on the batch at the current epoch's learning rate.  Returns the loss (both parts) before the update."""
        try:
            loss = self._update(left_names, right_names, overlaps, yaw_bins)
        finally:
            self._weights_changed()
        return float(loss)

    def fit(self, left_names, right_names, overlaps, yaw_bins, epochs: int, batch_size: Optional[int] = None, seed: int = 0) -> List[float]:
        """`epochs` passes over the pairs in shuffled mini-batches (`epoch_batches`; batch_size defaults to infer.batch_size).
        Returns the loss of every step."""
        ln, rn = [str(v) for v in left_names], [str(v) for v in right_names]
        ov = np.asarray(overlaps, np.float32).reshape(-1)
        yb = np.asarray(yaw_bins, np.int32).reshape(-1)
        if not (len(ln) == len(rn) == len(ov) == len(yb)) or len(ln) == 0:
            raise ValueError("fit: %d left, %d right names, %d overlaps and %d yaw bins" % (len(ln), len(rn), len(ov), len(yb)))
        bs = int(self.infer.batch_size if batch_size is None else batch_size)
        losses = []
        try:
            for _ in range(int(epochs)):
                for b in epoch_batches(len(ln), bs, self.epoch, seed):
                    losses.append(self._update([ln[i] for i in b], [rn[i] for i in b], ov[b], yb[b]))
                self.epoch += 1
        finally:
            self._weights_changed()
        return [float(v) for v in torch.cat(losses).cpu()] if losses else []

    def fit_from_npz(self, npz_files: Sequence[str], epochs: int, batch_size: Optional[int] = None, seed: int = 0,
                     no_pairs: Optional[int] = None) -> List[float]:
        """`fit` on the pairs of the reference's ground-truth npz files (evaluate.load_pairs) with the roles of evaluate.run_test:
        imgf1 -> head-left, imgf2 -> head-right, column 3 the yaw bin."""
        from .evaluate import load_pairs
        f1, f2, _d1, _d2, ov, yaw = load_pairs(npz_files, shuffle=False)
        n = len(f1) if no_pairs is None else min(int(no_pairs), len(f1))
        if n == 0:
            raise Exception("no training pairs")
        return self.fit(f1[:n], f2[:n], ov[:n], np.asarray(yaw[:n]).astype(np.int32), epochs, batch_size, seed)

    # -- results ------------------------------------------------------------------------------------
    def weights(self) -> Dict[str, np.ndarray]:
        """The full weight dict by Keras layer name as trained (negateDiffs undone: the file's c_conv1 kernel)."""
        out = dict(self.infer._weights)
        shapes = list(self.engine.head_param_shapes()) + list(self.engine.leg_param_shapes())
        for name, p, shape in zip(self.names, self.params, shapes):
            a = p.detach().cpu().numpy().reshape(shape).copy()
            out[name] = -a if (name == "c_conv1/kernel" and self.engine.negate_diffs) else a
        return out

    def save(self, path: str) -> None:
        """Write `weights()` as npz; the file loads through config['pretrained_weightsfilename']."""
        W.save_npz(path, self.weights())


class DataParallelTrainer(OverlapNetTrainer):
    """`OverlapNetTrainer` on every GPU of a node: one process per GPU (torch.distributed; `group` None = the default group), each
    with an ordinary, UNSHARDED `Infer` holding the same weights.  `step`, `fit` and `fit_from_npz` take the GLOBAL batch,
    identically on every rank (`epoch_batches` depends on (seed, epoch) alone, batch_size is the global one); rank r runs the chain
    of the base class on pairs `distributed.shard_bounds(len(batch), world, r)` of it, in order, over the unique scans of ITS pairs
    (a scan two ranks need is run by both).  The ranks' flat gradients [head | leg] meet in ONE all-gather
    (`distributed.exchange_gradients`), and one kernel (`OvnEngine.grad_reduce_adagrad`, csrc/grad_reduce.hip) forms
    g = float32(sum_r (n_r / n) g_r), in fp64 and rank order, and applies Adagrad to ONE flat parameter buffer and ONE flat
    accumulator, of which `params` / `accum` (names order; c_conv1/kernel as registered) are views.

    A rank that gets no pair (the last, partial batch of an epoch can have fewer pairs than ranks) runs no engine call and sends
    weight 0.  If the chain of any rank raises, that rank still enters the collective with a status; EVERY rank then raises
    `OvnError` naming the failed ranks, and no parameter or accumulator has moved anywhere.

    The same (seed, world) gives the same bits on every run and on every rank, whatever the backend: the reduction has a fixed
    order and no atomics, and does not depend on the order in which the collective delivers the rows.  Another `world` regroups a sum
    of float32-rounded per-rank means: it agrees to rounding, not bit for bit.  At world 1 the gradients are `OverlapNetTrainer`'s
    bits (one row, weight 1.0).  The post-conditions of the base class hold on every rank; `weights()` / `save()` work on any rank."""

    def __init__(self, infer, learning_rate: float, lr_alpha: float = 0.99, loss: str = "sigmoid", overlap_scale: float = 5.0,
                 yaw_scale: float = 1.0, min_overlap_for_angle: float = 0.7, train_legs: bool = True, group=None):
        import os
        import torch.distributed as dist
        if getattr(infer, "_world", 1) > 1:
            raise OvnError("DataParallelTrainer: not available on a sharded Infer (world %d): every rank takes an unsharded one" % infer._world)
        self.group = group
        if dist.is_available() and dist.is_initialized():
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        else:
            if group is not None or int(os.environ.get("WORLD_SIZE", "1")) > 1:
                raise OvnError("DataParallelTrainer: torch.distributed is not initialised (init_process_group first)")
            self.world, self.rank = 1, 0
        super().__init__(infer, learning_rate, lr_alpha, loss, overlap_scale, yaw_scale, min_overlap_for_angle, train_legs)
        if self.world > self.engine.GRAD_REDUCE_MAX_WORLD:
            raise OvnError("DataParallelTrainer: at most %d ranks, got %d" % (self.engine.GRAD_REDUCE_MAX_WORLD, self.world))
        # the tensors of the base class become views of one flat buffer each, in `names` order
        sizes = [int(p.numel()) for p in self.params]
        self.flat_params = torch.cat([p.reshape(-1) for p in self.params])
        self.flat_accum = torch.zeros_like(self.flat_params)
        offs = np.concatenate([[0], np.cumsum(sizes)])
        self.params = [self.flat_params[a:a + s].view(p.shape) for a, s, p in zip(offs, sizes, self.params)]
        self.accum = [self.flat_accum[a:a + s].view(p.shape) for a, s, p in zip(offs, sizes, self.params)]
        self.count = int(offs[-1] if self.train_legs else offs[8])       # elements exchanged and updated
        self._idle = torch.zeros(self.count, dtype=torch.float32, device=self.engine.device)     # what a rank without a gradient sends

    # -- one exchange -------------------------------------------------------------------------------
    def _exchange(self, left_names, right_names, overlaps, yaw_bins):
        """This rank's share of the global batch through the chain, then the all-gather.  -> (rows, rank weights, loss, r)."""
        from .distributed import exchange_gradients, shard_bounds
        ln, rn = [str(v) for v in left_names], [str(v) for v in right_names]
        ov = np.asarray(overlaps.cpu() if isinstance(overlaps, torch.Tensor) else overlaps, np.float32).reshape(-1)
        yb = np.asarray(yaw_bins.cpu() if isinstance(yaw_bins, torch.Tensor) else yaw_bins, np.int32).reshape(-1)
        if not (len(ln) == len(rn) == len(ov) == len(yb)) or not ln:
            raise ValueError("%d left, %d right names, %d overlaps and %d yaw bins (at least one pair)" % (len(ln), len(rn), len(ov), len(yb)))
        lo, hi = shard_bounds(len(ln), self.world, self.rank)
        flat, lv, status, err, r = self._idle, (0.0, 0.0), 0, None, None
        if hi > lo:
            try:
                r, grads = self._chain(ln[lo:hi], rn[lo:hi], ov[lo:hi], yb[lo:hi])
                flat = torch.cat([g.reshape(-1) for g in grads])
                lv = [float(v) for v in r["loss"].cpu()]
            except Exception as e:           # still enter the collective: the others must not wait for this rank
                flat, status, err = self._idle, 1, e
        rows, w, loss, statuses = exchange_gradients(flat, hi - lo, lv, status, self.group)
        bad = [int(k) for k in np.flatnonzero(statuses != 0)]
        if bad:
            raise OvnError("DataParallelTrainer: the chain of rank(s) %s failed, no weight moved%s"
                           % (bad, "" if err is None else " (this rank: %s)" % err)) from err
        return rows, w, loss, r

    def gradients(self, left_names, right_names, overlaps, yaw_bins) -> Dict[str, torch.Tensor]:
        """The reduced gradients of the GLOBAL batch with respect to the tensors of the weight FILE, by Keras name (the same bits on
        every rank), plus the global 'loss_overlap' and 'loss_yaw' (float64, 0-dim, host).  No update."""
        from .distributed import unpack_grad_trailer
        rows, w, _loss, _r = self._exchange(left_names, right_names, overlaps, yaw_bins)
        flat = self.engine.grad_reduce_adagrad(rows, w, count=self.count)
        out, off = {}, 0
        for name, p in zip(self.names, self.params):
            if off >= self.count:
                break
            g = flat[off:off + p.numel()].view(p.shape)
            out[name] = -g if (name == "c_conv1/kernel" and self.engine.negate_diffs) else g
            off += p.numel()
        lss = unpack_grad_trailer(rows)[0]
        for k, key in enumerate(("loss_overlap", "loss_yaw")):
            out[key] = torch.tensor(sum(w[r] * lss[r, k] for r in range(self.world) if w[r] != 0.0), dtype=torch.float64)
        return out

    def _update(self, left_names, right_names, overlaps, yaw_bins) -> torch.Tensor:
        rows, w, loss, r = self._exchange(left_names, right_names, overlaps, yaw_bins)
        self.engine.grad_reduce_adagrad(rows, w, self.flat_params[:self.count], self.flat_accum[:self.count],
                                        float(lr_schedule(self.epoch, self.learning_rate, self.lr_alpha)))
        self.engine.set_head_weights(self.params[:8])
        if self.train_legs:
            self.engine.set_leg_weights(dict(zip(self.leg_names, self.params[8:])))
        self.last = r
        return torch.tensor([loss], dtype=torch.float64)
