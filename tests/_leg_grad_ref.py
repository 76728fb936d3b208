"""TEST INFRASTRUCTURE: the leg restated in torch with forced ReLU masks, x_{l+1} = mask_l * (conv_l(x_l) + b_l), in any dtype and
differentiated by autograd -- the yardstick of `ovn_leg_backward` / `ovn_debug_conv_grad` (csrc/leg_backward.hip) -- the
whole-network composition with tests/_feature_grad_ref.py, and the fixtures the host and GPU tests share.

Without forced masks mask_l = [pre_l > 0], which is the ReLU (tests/test_leg_train_host.py pins that to
oracle.overlapnet_oracle.leg_forward, the gradients to central differences, and the end-to-end derivative of the whole network to the
chained form `train.OverlapNetTrainer` uses)."""
import numpy as np
import torch

from overlapnet_amd import weights as WT
from tests import _feature_grad_ref as F
from tests import _head_grad_ref as R

SCAN_BLOCK = 4        # OVN_LEG_GRAD_SCAN_BLOCK (tests/test_leg_train_host.py checks it against the header)


def leg_names(in_c, cfg=None):
    return [l.name + "/" + kind for l in WT.leg_layers(in_c, cfg) for kind in ("kernel", "bias")]


def _conv_nchw(x, kernel, bias, stride, mask=None):
    """The oracle's convolution call (contiguous NCHW input, (cout, cin, kh, kw) kernel) followed by the mask (NHWC, or None: ReLU)."""
    pre = torch.nn.functional.conv2d(x, kernel.permute(3, 2, 0, 1).contiguous(), bias, stride=stride, padding=0)
    m = (pre > 0) if mask is None else torch.as_tensor(np.asarray(mask)).permute(0, 3, 1, 2).to(torch.bool)
    return torch.where(m, pre, torch.zeros((), dtype=pre.dtype)), pre


def conv_layer(x, kernel, bias, stride, mask=None):
    """One layer on x (n, h, w, cin) (torch, channels last): mask * (conv(x) + b); mask None: [pre > 0].  -> (out, pre), channels last."""
    y, pre = _conv_nchw(x.permute(0, 3, 1, 2).contiguous(), kernel, bias, stride, mask)
    return y.permute(0, 2, 3, 1), pre.permute(0, 2, 3, 1)


def leg_forward(params, x, layers, masks=None):
    """params: [k0, b0, k1, b1, ...] tensors; x (n, H, W, C) tensor -> the list of every layer's output (n, oh, ow, cout)."""
    acts = []
    x = x.permute(0, 3, 1, 2).contiguous()
    for li, l in enumerate(layers):
        x, _ = _conv_nchw(x, params[2 * li], params[2 * li + 1], (l.sh, l.sw), None if masks is None else masks[li])
        acts.append(x.permute(0, 2, 3, 1))
    return acts


def layer_grads(kernel, bias, x, out_mask, dout, stride, dtype=torch.float64):
    """The three gradients of sum(dout * mask * (conv(x) + b)) -> dict of numpy din, dkernel, dbias."""
    k = torch.tensor(np.asarray(kernel), dtype=dtype, requires_grad=True)
    b = torch.tensor(np.asarray(bias), dtype=dtype, requires_grad=True)
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    y, _ = conv_layer(xt, k, b, stride, out_mask)
    g = torch.autograd.grad((y * torch.tensor(np.asarray(dout), dtype=dtype)).sum(), [xt, k, b])
    return {"din": g[0].numpy(), "dkernel": g[1].numpy(), "dbias": g[2].numpy()}


def leg_grads(weights, images, dfeat, cfg=None, dtype=torch.float64, masks=None):
    """Gradients of sum(dfeat * feature volumes) with respect to the leg tensors -> (dict name -> numpy gradient, list of the
    activations as numpy).  images (n, H, W, C); dfeat (n, W, 128)."""
    images = np.asarray(images)
    layers = WT.leg_layers(images.shape[3], cfg)
    names = leg_names(images.shape[3], cfg)
    params = [torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=True) for k in names]
    acts = leg_forward(params, torch.tensor(images, dtype=dtype), layers, masks)
    d = torch.tensor(np.asarray(dfeat), dtype=dtype).reshape(acts[-1].shape)
    g = torch.autograd.grad((acts[-1] * d).sum(), params)
    return {k: v.numpy() for k, v in zip(names, g)}, [a.detach().numpy() for a in acts]


def network_loss(weights, images, lidx, ridx, targets, bins, s, cfg=None, loss="sigmoid", overlap_scale=5.0, yaw_scale=1.0,
                 threshold=F.THRESHOLD, dtype=torch.float64, negate=False, leg_masks=None, head_masks=None, grad=True):
    """The whole Siamese network end to end: the shared leg on the unique scans `images` (k, H, W, C), pair p = (features[lidx[p]],
    features[ridx[p]]), both losses.  -> dict: 'loss_overlap', 'loss_yaw', 'acts' (numpy list), 'pre2', 'pre3', 'y', and with grad
    'grads': name -> gradient of the sum of both losses for all 8 + 2 x layers tensors (with respect to the tensors in the FILE)."""
    images = np.asarray(images)
    layers = WT.leg_layers(images.shape[3], cfg)
    lnames = leg_names(images.shape[3], cfg)
    lp = [torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=grad) for k in lnames]
    hp = [torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=grad) for k in R.HEAD_PARAMS]
    t = torch.tensor(np.asarray(targets), dtype=dtype)
    with torch.set_grad_enabled(grad):
        acts = leg_forward(lp, torch.tensor(images, dtype=dtype), layers, leg_masks)
        feats = acts[-1].reshape(images.shape[0], -1, 128)
        n, W = len(lidx), feats.shape[1]
        lt, rt = feats[list(lidx)], feats[list(ridx)]
        qt = torch.tensor(F.yaw_targets(bins, targets, W, threshold), dtype=dtype)
        hm = None if head_masks is None else [torch.as_tensor(np.asarray(m)) for m in head_masks]
        f = R.forward(hp, lt, rt, s, negate, hm)
        lov = (overlap_scale / n) * R.loss_terms(f["y"], t, loss).sum()
        lyaw = (yaw_scale / (n * W)) * F.yaw_loss_terms(F.corr_logits(lt, rt), qt, W).sum()
    out = {"loss_overlap": float(lov.detach()), "loss_yaw": float(lyaw.detach()), "acts": [a.detach().numpy() for a in acts],
           "pre2": f["pre2"].detach().numpy(), "pre3": f["pre3"].detach().numpy(), "y": f["y"].detach().numpy()}
    if grad:
        g = torch.autograd.grad(lov + lyaw, hp + lp)
        out["grads"] = {k: v.numpy() for k, v in zip(list(R.HEAD_PARAMS) + lnames, g)}
    return out


def chained_grads(weights, images, lidx, ridx, targets, bins, s, cfg=None, loss="sigmoid", dtype=torch.float64):
    """The same gradients the way the trainer forms them: leg forward, `feature_loss` per pair, the rows summed per scan for both
    sides, leg backward from that sum."""
    images = np.asarray(images)
    layers = WT.leg_layers(images.shape[3], cfg)
    lnames = leg_names(images.shape[3], cfg)
    with torch.no_grad():
        lp = [torch.tensor(np.asarray(weights[k]), dtype=dtype) for k in lnames]
        feats = leg_forward(lp, torch.tensor(images, dtype=dtype), layers)[-1].reshape(images.shape[0], -1, 128).numpy()
    fl = F.feature_loss(weights, feats[list(lidx)], feats[list(ridx)], targets, bins, s, loss, dtype=dtype)
    dfeat = np.zeros_like(feats)
    np.add.at(dfeat, list(lidx), fl["dl"]["both"])
    np.add.at(dfeat, list(ridx), fl["dr"]["both"])
    g, _ = leg_grads(weights, images, dfeat, cfg, dtype)
    g.update(fl["grads"])
    return g


# --------------------------------------------------------------------------------------------------------------------------------
# Fixtures
# --------------------------------------------------------------------------------------------------------------------------------

def make_images(rng, n, h, w, c):
    """Leg inputs like the cue images: depth-like positive values with empty pixels (-1), normals in [-1, 1]."""
    x = rng.uniform(-1.0, 1.0, (n, h, w, c)).astype(np.float32)
    x[..., 0] = rng.uniform(0.5, 40.0, (n, h, w)).astype(np.float32)
    x[rng.random((n, h, w)) < 0.1] = -1.0
    return x


def leg_weights(in_c, cfg=None, seed=0, feat_w=45):
    """Seeded weights whose leg keeps about half of its units alive down to the last layer (Glorot kernels with a gain, small biases)."""
    return WT.synthetic_weights(in_c, cfg, seed=seed, kernel_gain=1.4, feat_w=feat_w, gains={"overlap_output": R.DENSE_GAIN})


def random_dfeat(rng, feats):
    """dL/d(feature volumes): random, given to every unit alive or dead (the masks must remove the dead ones' share)."""
    return rng.normal(0.0, 1.0, feats.shape).astype(np.float32)


# The trainer fixture: the 32 x 247 leg (W = 45, s = 15), 6 scans, 8 pairs with a scan that is left in one pair and right in another,
# a fixed batch stepped TRAINER["steps"] times
TRAINER = {"W": 45, "s": 15, "scans": 6, "lr": 2e-3, "alpha": 0.99, "steps": 4, "loss": "sigmoid", "seed": 0,
           "left": [0, 1, 2, 3, 4, 5, 1, 0], "right": [1, 2, 0, 4, 5, 3, 1, 3], "bins": [0, 44, 22, 7, 30, 12, 22, 40]}


def trainer_inputs():
    t = TRAINER
    h, w = R.GEOMS[(t["W"], t["s"])]
    rng = np.random.default_rng([t["seed"], 2021])
    cfg = R.model_cfg(t["W"], t["s"])
    images = make_images(rng, t["scans"], h, w, 4)
    images[..., 0] /= 40.0                      # depth scaled to [0, 1]: keeps the correlation logits off saturation
    weights = leg_weights(4, cfg, t["seed"], t["W"])
    teacher = leg_weights(4, cfg, t["seed"] + 1, t["W"])
    tr = network_loss(teacher, images, t["left"], t["right"], np.zeros(len(t["left"])), t["bins"], t["s"], cfg, grad=False)
    targets = tr["y"].astype(np.float32)
    targets[0], targets[1] = 0.9, 0.2           # pairs on both sides of min_overlap_for_angle
    return {"cfg": cfg, "images": images, "weights": weights, "targets": targets, "left": t["left"], "right": t["right"],
            "bins": np.asarray(t["bins"], np.int32)}


_TRAINER_LOSSES = []


def trainer_losses64():
    """fp64 CPU: the fixed batch's loss before each of TRAINER['steps'] Adagrad steps on all 30 tensors, and after the last."""
    if _TRAINER_LOSSES:
        return _TRAINER_LOSSES
    from overlapnet_amd.train import adagrad_step, lr_schedule
    t, x = TRAINER, trainer_inputs()
    names = list(R.HEAD_PARAMS) + leg_names(4, x["cfg"])
    params = [torch.tensor(np.asarray(x["weights"][k]), dtype=torch.float64) for k in names]
    accum = [torch.zeros_like(p) for p in params]
    for step in range(t["steps"] + 1):
        w = {k: p.numpy() for k, p in zip(names, params)}
        r = network_loss(w, x["images"], x["left"], x["right"], x["targets"], x["bins"], t["s"], x["cfg"], t["loss"],
                         grad=step < t["steps"])
        _TRAINER_LOSSES.append(r["loss_overlap"] + r["loss_yaw"])
        if step < t["steps"]:
            adagrad_step(params, accum, [torch.tensor(r["grads"][k]) for k in names], float(lr_schedule(0, t["lr"], t["alpha"])))
    return _TRAINER_LOSSES
