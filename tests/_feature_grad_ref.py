"""TEST INFRASTRUCTURE: both heads' losses restated in torch for any (W, s) and any dtype, differentiated by autograd down to the
feature volumes -- the yardstick of `ovn_heads_feature_grad` (csrc/heads_feature_grad.hip) -- and the fixtures the host and GPU tests
share.

The Delta part is tests/_head_grad_ref.forward (forced ReLU masks included); the correlation logits, the yaw target and the
weighted cross entropy follow NormalizedCorrelation2D.py:75-109 + RangePadding2D, ImagePairOverlapOrientationSequence.py:118-121 and
training.py:86-92 of the reference:
    z_p[k] = sum_{j, c} l_p[(k + j + W // 2) mod W, c] r_p[j, c]
    q_p[k] = [k == bin_p and t_p > min_overlap_for_angle],  m = 1 + (W - 1) q
    L_yaw  = yaw_scale / (n W) sum_{p, k} (1 - q) z + m (log1p(exp(-|z|)) + max(-z, 0))
The leaves are the per-pair volumes l, r (n, W, 128) and the eight head tensors.  `feature_loss` runs ONE forward and differentiates
the two losses separately, so the overlap-only, yaw-only and combined gradients of a case come from the same evaluation (combined =
the sum, in the dtype of the run, as autograd's own accumulation would form it).

Fixtures: the geometries, weights and volumes of _head_grad_ref.CASES, plus yaw bins and targets per case.  The volumes are scaled
by a per-case power of two so that the correlation logits (sums of W x 128 non-negative products, about 10^3 .. 10^4 unscaled) land
around 3: unsaturated.  tests/test_feature_grad_host.py guards all of this."""
import numpy as np
import torch

from tests import _head_grad_ref as R

CASES = R.CASES
THRESHOLD = 0.7
SELF_PAIR_CASE = (45, 15, 3, "idx", "mse")       # its pair 1 has lidx == ridx on a volume of equal rows: every sign is zero
LOGIT_TARGET = 3.0                               # median logit after scaling, within a factor sqrt(2) either way


def corr_logits(l, r):
    """(n, W, 128) x (n, W, 128) torch tensors -> z (n, W)."""
    n, W, _ = l.shape
    m = torch.einsum("nic,njc->nij", l, r)
    jj = torch.arange(W)
    idx = (torch.arange(W)[:, None] + jj[None, :] + W // 2) % W
    return m[:, idx, jj[None, :]].sum(dim=2)


def yaw_targets(bins, targets, W, threshold=THRESHOLD):
    """q (n, W) float64 numpy: one-hot of the bin where the overlap target exceeds the threshold (compared in float32, as the library
    does) and the bin lies in [0, W); zeros otherwise."""
    q = np.zeros((len(bins), W))
    t = np.asarray(targets, np.float32)
    for p, b in enumerate(bins):
        if 0 <= int(b) < W and t[p] > np.float32(threshold):
            q[p, int(b)] = 1.0
    return q


def yaw_loss_terms(z, q, W):
    """TF's weighted_cross_entropy_with_logits(targets=q, logits=z, pos_weight=W), elementwise."""
    return (1.0 - q) * z + (1.0 + (W - 1.0) * q) * (torch.log1p(torch.exp(-torch.abs(z))) + torch.relu(-z))


def feature_loss(weights, l, r, targets, bins, s, loss="sigmoid", overlap_scale=5.0, yaw_scale=1.0, threshold=THRESHOLD,
                 dtype=torch.float64, negate=False, masks=None, grad=True):
    """-> dict of numpy arrays: the stage values of _head_grad_ref.forward, 'z' (n, W), 'q', 'loss_overlap', 'loss_yaw', and with
    grad: 'dl' / 'dr' = {'overlap', 'yaw', 'both'} -> (n, W, 128), 'dz' = d L_yaw / d z (n, W), 'grads' (the head tensors' gradients
    of the overlap loss, by name)."""
    params = [torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=grad) for k in R.HEAD_PARAMS]
    lt = torch.tensor(np.asarray(l), dtype=dtype, requires_grad=grad)
    rt = torch.tensor(np.asarray(r), dtype=dtype, requires_grad=grad)
    t = torch.tensor(np.asarray(targets), dtype=dtype)
    n, W, _ = lt.shape
    q = yaw_targets(bins, targets, W, threshold)
    qt = torch.tensor(q, dtype=dtype)
    if masks is not None:
        masks = [torch.as_tensor(np.asarray(m)) for m in masks]
    with torch.set_grad_enabled(grad):
        f = R.forward(params, lt, rt, s, negate, masks)
        lov = (overlap_scale / n) * R.loss_terms(f["y"], t, loss).sum()
        z = corr_logits(lt, rt)
        lyaw = (yaw_scale / (n * W)) * yaw_loss_terms(z, qt, W).sum()
    out = {k: v.detach().numpy() for k, v in f.items()}
    out.update({"z": z.detach().numpy(), "q": q, "loss_overlap": float(lov.detach()), "loss_yaw": float(lyaw.detach())})
    if grad:
        gov = torch.autograd.grad(lov, [lt, rt] + params, retain_graph=True)
        gy = torch.autograd.grad(lyaw, [lt, rt, z])
        out["dl"] = {"overlap": gov[0].numpy(), "yaw": gy[0].numpy(), "both": (gov[0] + gy[0]).numpy()}
        out["dr"] = {"overlap": gov[1].numpy(), "yaw": gy[1].numpy(), "both": (gov[1] + gy[1]).numpy()}
        out["dz"] = gy[2].numpy()
        out["grads"] = {k: g.numpy() for k, g in zip(R.HEAD_PARAMS, gov[2:])}
    return out


def pool_scale_grad(weights, pool, lidx, ridx, targets, bins, s, loss="sigmoid", overlap_scale=5.0, yaw_scale=1.0,
                    threshold=THRESHOLD, dtype=torch.float64, masks=None):
    """The yardstick of `train.heads_loss`: the pools are a * pool for a leaf a (k, 1, 1) of ones, pair p reads entries lidx[p] and
    ridx[p] of it; -> (L_ov + L_yaw, d (L_ov + L_yaw) / d a as a (k) array)."""
    params = [torch.tensor(np.asarray(weights[k]), dtype=dtype) for k in R.HEAD_PARAMS]
    a = torch.ones((pool.shape[0], 1, 1), dtype=dtype, requires_grad=True)
    x = a * torch.tensor(np.asarray(pool), dtype=dtype)
    lt, rt = x[list(lidx)], x[list(ridx)]
    n, W, _ = lt.shape
    t = torch.tensor(np.asarray(targets), dtype=dtype)
    qt = torch.tensor(yaw_targets(bins, targets, W, threshold), dtype=dtype)
    if masks is not None:
        masks = [torch.as_tensor(np.asarray(m)) for m in masks]
    f = R.forward(params, lt, rt, s, False, masks)
    total = (overlap_scale / n) * R.loss_terms(f["y"], t, loss).sum() \
        + (yaw_scale / (n * W)) * yaw_loss_terms(corr_logits(lt, rt), qt, W).sum()
    total.backward()
    return float(total.detach()), a.grad.reshape(-1).numpy()


# --------------------------------------------------------------------------------------------------------------------------------
# Fixtures
# --------------------------------------------------------------------------------------------------------------------------------

_CASES = {}


def make_case(case_key):
    """_head_grad_ref.make_case plus: 'bins' (n) int32, 'targets' (n) float32 with pairs on both sides of the threshold, 'scale' (the
    power of two the volumes were multiplied by); SELF_PAIR_CASE gets ridx[1] = lidx[1] on an entry of equal rows.  Cached; treat as read-only."""
    if case_key in _CASES:
        return _CASES[case_key]
    W, s, n, form, loss = case_key
    ci = CASES.index(case_key)
    c = dict(R.make_case(*case_key))
    rng = np.random.default_rng([7, ci])
    if case_key == SELF_PAIR_CASE:      # pair 1 = (e, e) on an entry whose rows are all equal: l[i, c] - r[j, c] = 0 for every i, j
        c["ridx"] = list(c["ridx"])
        c["ridx"][1] = c["lidx"][1]
        c["pool"] = c["pool"].copy()
        c["pool"][c["lidx"][1]] = c["pool"][c["lidx"][1]][:1]
    # targets: the head's, with one pair above and one at or below the threshold (n = 1: above for even case numbers)
    t = np.array(c["targets"], np.float32)
    if n >= 2:
        if not np.any(t > THRESHOLD):
            t[0] = 0.85
        if not np.any(t <= THRESHOLD):
            t[1] = 0.30
    elif ci % 2 == 0:
        t[0] = 0.90
    c["targets"] = t
    # bins: 0, W - 1 and W // 2 in turn over cases and pairs, then random ones
    edge = [0, W - 1, W // 2]
    c["bins"] = np.array([edge[(ci + p) % 3] if p < 3 else int(rng.integers(0, W)) for p in range(n)], np.int32)

    def gather(pool, right):
        if form == "idx":
            return pool[c["lidx"]], pool[c["ridx"]]
        return pool[:n], np.repeat(right[:1], n, axis=0)
    l0, r0 = gather(c["pool"], c["right"])
    z0 = corr_logits(torch.tensor(l0, dtype=torch.float64), torch.tensor(r0, dtype=torch.float64)).numpy()
    a = np.float32(2.0 ** round(0.5 * np.log2(LOGIT_TARGET / float(np.median(z0)))))
    c["scale"] = float(a)
    c["pool"] = c["pool"] * a
    c["right"] = c["pool"] if form == "idx" else c["right"] * a
    c["l"], c["r"] = gather(c["pool"], c["right"])
    _CASES[case_key] = c
    return c


_REF = {}


def reference(case_key, grad=True):
    """The case and its fp64 `feature_loss` without forced masks (overlap_scale 5, yaw_scale 1); grad False: the forward alone, for
    the tests that only need the pre-activations.  Cached."""
    c = make_case(case_key)
    if (case_key, True) in _REF:
        return c, _REF[(case_key, True)]
    if (case_key, grad) not in _REF:
        _REF[(case_key, grad)] = feature_loss(c["weights"], c["l"], c["r"], c["targets"], c["bins"], c["s"], c["loss"], grad=grad)
    return c, _REF[(case_key, grad)]
