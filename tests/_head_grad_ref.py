"""TEST INFRASTRUCTURE: the Delta head restated in torch for any (W, s), differentiated by autograd -- the yardstick of
`ovn_delta_head_grad` (csrc/delta_head_backward.hip) -- and the seeded fixtures the host and GPU tests share.

`head_loss` materialises |l - r| (a few rows of l at a time: at W = 360 a pair's difference tensor is 130 MB in fp64), runs
c_conv1 (linear), c_conv2 + ReLU, c_conv3 + ReLU, Dense, sigmoid and the loss  scale / n * sum_p loss(y_p, t_p)  in the dtype it is
given (float64: the reference; float32 on the CPU: the yardstick of what fp32 summation in another order costs), and returns the
stage values, the loss and the eight gradients in Keras layouts.  Optional forced ReLU masks replace [pre > 0] of o2 / o3, so that
gradients can be compared on the branch another evaluation took.  tests/test_head_train_host.py pins the forward to
oracle.error_bounds.head_pair and the gradients to central differences."""
import numpy as np
import torch

from oracle import error_bounds as E
from overlapnet_amd import weights as WT

HEAD_PARAMS = ("c_conv1/kernel", "c_conv1/bias", "c_conv2/kernel", "c_conv2/bias", "c_conv3/kernel", "c_conv3/bias",
               "overlap_output/kernel", "overlap_output/bias")
PAIR_BLOCK = 4        # OVN_GRAD_PAIR_BLOCK (tests/test_head_train_host.py checks it against the header)


def loss_terms(y, t, loss):
    """Per-pair loss: 'sigmoid' = the reference's my_sigmoid_loss (training.py:71-83), 'mse' = squared error."""
    if loss == "sigmoid":
        return torch.sigmoid(24.0 * torch.abs(y - t) - 6.0)
    if loss == "mse":
        return (y - t) ** 2
    raise ValueError(loss)


def forward(params, l, r, s, negate=False, masks=None, rows=64):
    """params: the eight tensors (HEAD_PARAMS order, Keras shapes); l, r: (n, W, 128) tensors of the same dtype, pair p = (l[p], r[p]).
    Returns dict of o1 (n, W, G, 64), pre2 / o2 (n, G, G, 128), pre3 / o3 (n, H, H, 256), logit (n), y (n).  masks = (m2, m3): 0 / 1
    tensors used instead of [pre > 0]."""
    w1, b1, w2, b2, w3, b3, wd, bd = params
    n, wd_, _ = l.shape
    g = wd_ // s
    R = g * s
    w1m = w1.reshape(s * 128, 64)
    o1 = []
    for p in range(n):
        blocks = []
        for i0 in range(0, wd_, rows):
            d = torch.abs(l[p, i0:i0 + rows, None, :] - r[p, None, :R, :])
            if negate:
                d = -d
            blocks.append(d.reshape(-1, g, s * 128) @ w1m + b1)
        o1.append(torch.cat(blocks))
    o1 = torch.stack(o1)                                                    # (n, W, G, 64)
    x = o1[:, :R].reshape(n, g, s, g, 64).permute(0, 1, 3, 2, 4).reshape(n, g, g, s * 64)
    pre2 = x @ w2.reshape(s * 64, 128) + b2
    m2 = (pre2 > 0).to(pre2.dtype) if masks is None else masks[0].to(pre2.dtype)
    o2 = pre2 * m2
    pre3 = torch.nn.functional.conv2d(o2.permute(0, 3, 1, 2), w3.permute(3, 2, 0, 1), b3).permute(0, 2, 3, 1)
    m3 = (pre3 > 0).to(pre3.dtype) if masks is None else masks[1].to(pre3.dtype)
    o3 = pre3 * m3
    logit = o3.reshape(n, -1) @ wd.reshape(-1) + bd.reshape(())
    return {"o1": o1, "pre2": pre2, "o2": o2, "pre3": pre3, "o3": o3, "logit": logit, "y": torch.sigmoid(logit)}


def head_loss(weights, l, r, targets, s, loss="sigmoid", scale=1.0, dtype=torch.float64, negate=False, masks=None, grad=True):
    """weights: dict by Keras layer name (numpy); l, r: (n, W, 128) arrays; targets (n).  Returns dict of numpy arrays: the stage
    values of `forward`, 'loss' and 'grads' (name of HEAD_PARAMS -> gradient in its Keras shape, with respect to the tensors in the
    FILE: under `negate` c_conv1 multiplies -|l - r|)."""
    params = [torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=grad) for k in HEAD_PARAMS]
    lt, rt = torch.tensor(np.asarray(l), dtype=dtype), torch.tensor(np.asarray(r), dtype=dtype)
    t = torch.tensor(np.asarray(targets), dtype=dtype)
    if masks is not None:
        masks = [torch.as_tensor(np.asarray(m)) for m in masks]
    with torch.set_grad_enabled(grad):
        f = forward(params, lt, rt, s, negate, masks)
        total = (scale / lt.shape[0]) * loss_terms(f["y"], t, loss).sum()
    out = {k: v.detach().numpy() for k, v in f.items()}
    out["loss"] = float(total.detach())
    if grad:
        gs = torch.autograd.grad(total, params)
        out["grads"] = {k: g.numpy() for k, g in zip(HEAD_PARAMS, gs)}
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# Fixtures shared by tests/test_head_train_host.py (the guard) and tests/test_gpu_head_train.py
# --------------------------------------------------------------------------------------------------------------------------------

# (W, s) -> input (H, W) of a leg that produces W columns (in_w = 2 W + 157 for the 32-row leg; 64 x 900 with
# additional_unsymmetric_layer3a at 360)
GEOMS = {(45, 15): (32, 247), (60, 15): (32, 277), (77, 15): (32, 311), (50, 16): (32, 257), (45, 10): (32, 247), (360, 15): (64, 900)}
# per small geometry: (n, index form, loss); 'idx' = lidx / ridx with repeats, '1vN' = ridx None
SMALL_CASES = ((1, "1vN", "sigmoid"), (3, "idx", "mse"), (PAIR_BLOCK + 1, "idx", "sigmoid"), (PAIR_BLOCK + 1, "1vN", "mse"))
CASES = [(W, s, n, form, loss) for (W, s) in GEOMS if W != 360 for (n, form, loss) in SMALL_CASES] + [(360, 15, 2, "idx", "sigmoid")]
DENSE_GAIN = 4.0      # Glorot alone keeps the logits within a few tenths of the bias; this spreads them over the sigmoid's slope
SEEDS = {(45, 10, 3, "idx", "mse"): 1}            # case -> seed, where seed 0 fails the guard of tests/test_head_train_host.py (an overlap below 0.02)


def model_cfg(W, s):
    from tools import synthetic as S
    h, w = GEOMS[(W, s)]
    return dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=W, additional_unsymmetric_layer3a=(W == 360),
                conv1NetworkHead_conv1size=s)


def make_weights(W, s, seed=0):
    return WT.synthetic_weights(4, model_cfg(W, s), seed=seed, gains={"overlap_output": DENSE_GAIN}, feat_w=W)


def make_case(W, s, n, form, loss, seed=None):
    """-> dict: weights, pool (k, W, 128) float32 (left volumes), right (kr, W, 128), lidx / ridx (lists or None), the gathered
    l / r (n, W, 128), targets (n) float32."""
    if seed is None:
        seed = SEEDS.get((W, s, n, form, loss), 0)
    rng = np.random.default_rng([seed, W, s, n])
    k = max(n, 3)
    vols = E._relu_vol(rng, k + 1, width=W)
    for v in vols:
        v[:, rng.choice(128, 8, replace=False)] = 0
    pool, right = vols[:k], vols[k:]
    if form == "idx":
        lidx = [int(v) for v in rng.integers(0, k, n)]
        ridx = [int(v) for v in rng.integers(0, k, n)]
        if n > 1:
            lidx[-1] = lidx[0]              # a repeat for certain
        right = pool
        l, r = pool[lidx], pool[ridx]
    else:
        lidx = ridx = None
        l, r = pool[:n], np.repeat(right[:1], n, axis=0)
    targets = rng.uniform(0, 1, n).astype(np.float32)
    return {"weights": make_weights(W, s, seed), "pool": pool, "right": right, "lidx": lidx, "ridx": ridx, "l": l, "r": r,
            "targets": targets, "W": W, "s": s, "n": n, "loss": loss, "form": form}


_REF = {}


def reference(case_key, dtype=torch.float64, masks=None, negate=False, scale=1.0):
    """Cached `head_loss` of a case of CASES (the fp64 reference without forced masks is shared by every test that needs it)."""
    c = make_case(*case_key)
    if masks is None and dtype == torch.float64 and not negate and scale == 1.0:
        if case_key not in _REF:
            _REF[case_key] = head_loss(c["weights"], c["l"], c["r"], c["targets"], c["s"], c["loss"])
        return c, _REF[case_key]
    return c, head_loss(c["weights"], c["l"], c["r"], c["targets"], c["s"], c["loss"], scale=scale, dtype=dtype, negate=negate, masks=masks)


def undecided(c, ref):
    """{'o2', 'o3'}: boolean tensors of the units whose fp64 pre-activation lies within the elementwise error bound of the fp32
    kernels (E.head_bounds, mode 'generic') of zero: an fp32 evaluation may land on either side of the ReLU there."""
    out = {"o2": np.zeros(ref["pre2"].shape, bool), "o3": np.zeros(ref["pre3"].shape, bool)}
    for p in range(c["n"]):
        h = E.head_pair(c["l"][p], c["r"][p], c["weights"], c["s"])
        b = E.head_bounds(h, c["weights"], "generic")
        out["o2"][p] = np.abs(ref["pre2"][p]) <= b["o2"]
        out["o3"][p] = np.abs(ref["pre3"][p]) <= b["o3"]
    return out


def undecided_fraction(c, ref):
    return {k: float(v.mean()) for k, v in undecided(c, ref).items()}


def overlap_bounds(c, ref):
    """Per pair: E.overlap_bound of the logit bound of the fp32 kernels."""
    out = []
    for p in range(c["n"]):
        h = E.head_pair(c["l"][p], c["r"][p], c["weights"], c["s"])
        out.append(E.head_bounds(h, c["weights"], "generic")["overlap"])
    return np.asarray(out)


LOSS_SLOPE = {"sigmoid": 6.0, "mse": 2.0}     # max |d loss / d y| over y, t in [0, 1]: 24 / 4 and 2 |y - t|


# --------------------------------------------------------------------------------------------------------------------------------
# The trainer's trajectory fixture: (45, 15), 32 pairs over 8 volumes, 3 epochs of 4 Adagrad steps (batch 8)
# --------------------------------------------------------------------------------------------------------------------------------

TRAJ = {"W": 45, "s": 15, "pairs": 32, "volumes": 8, "batch": 8, "epochs": 3, "lr": 1e-4, "alpha": 0.99, "loss": "sigmoid",
        "loss_weight": 5.0, "seed": 0}
_TRAJ = {}


def trajectory_inputs():
    t = TRAJ
    rng = np.random.default_rng([t["seed"], 77])
    vols = E._relu_vol(rng, t["volumes"], width=t["W"])
    for v in vols:
        v[:, rng.choice(128, 8, replace=False)] = 0
    left = rng.integers(0, t["volumes"], t["pairs"])
    right = rng.integers(0, t["volumes"], t["pairs"])
    # targets a head can reach: the overlaps of a "teacher" head with other seeded weights (uniform random targets carry no signal
    # the features explain, and the batch-to-batch scatter of the loss then hides the descent)
    teacher = make_weights(t["W"], t["s"], t["seed"] + 1)
    targets = head_loss(teacher, vols[left], vols[right], np.zeros(t["pairs"]), t["s"], grad=False)["y"].astype(np.float32)
    return {"weights": make_weights(t["W"], t["s"], t["seed"]), "vols": vols, "left": left, "right": right, "targets": targets}


def trajectory():
    """The fp64 CPU trajectory of the trainer test (train.adagrad_step on the reference's gradients, train.epoch_batches'
    mini-batches): per step the loss before the update, the batch, its overlaps, the own bound of the loss, and for how many
    steps an fp32 CPU run of the same recipe keeps the fp64 run's ReLU masks.  Cached."""
    if _TRAJ:
        return _TRAJ
    from overlapnet_amd.train import adagrad_step, epoch_batches, lr_schedule
    t, x = TRAJ, trajectory_inputs()
    runs = {}
    for dtype in (torch.float64, torch.float32):
        params = [torch.tensor(np.asarray(x["weights"][k]), dtype=dtype) for k in HEAD_PARAMS]
        accum = [torch.zeros_like(p) for p in params]
        steps = []
        for epoch in range(t["epochs"]):
            for b in epoch_batches(t["pairs"], t["batch"], epoch, t["seed"]):
                w = {k: p.numpy() for k, p in zip(HEAD_PARAMS, params)}
                l, r = x["vols"][x["left"][b]], x["vols"][x["right"][b]]
                ref = head_loss(w, l, r, x["targets"][b], t["s"], t["loss"], scale=t["loss_weight"], dtype=dtype)
                step = {"batch": b, "loss": ref["loss"], "y": ref["y"], "m2": ref["pre2"] > 0, "m3": ref["pre3"] > 0}
                if dtype == torch.float64:      # own bound of this step's loss: loss_weight * slope * mean overlap bound
                    c = {"weights": {k: w[k] for k in HEAD_PARAMS}, "l": l, "r": r, "s": t["s"], "n": len(b)}
                    step["ybound"] = overlap_bounds(c, ref)
                    step["own"] = t["loss_weight"] * LOSS_SLOPE[t["loss"]] * float(step["ybound"].mean())
                steps.append(step)
                grads = [torch.tensor(ref["grads"][k], dtype=dtype) for k in HEAD_PARAMS]
                adagrad_step(params, accum, grads, float(lr_schedule(epoch, t["lr"], t["alpha"])))
        runs[dtype] = steps
    s64, s32 = runs[torch.float64], runs[torch.float32]
    same = 0
    for a, b in zip(s64, s32):
        if not (np.array_equal(a["m2"], b["m2"]) and np.array_equal(a["m3"], b["m3"])):
            break
        same += 1
    _TRAJ.update({"steps": s64, "losses64": [s["loss"] for s in s64], "losses32": [s["loss"] for s in s32],
                  "steps_with_equal_masks": same, "bound": list(np.cumsum([s["own"] for s in s64]))})
    return _TRAJ
