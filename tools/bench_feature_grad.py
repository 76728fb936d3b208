"""Time of one call of the feature-gradient path (`OvnEngine.heads_feature_grad` -> ovn_heads_feature_grad,
csrc/heads_feature_grad.hip) on 16 pairs at feature widths 360 (64 x 900) and 371 (32 x 900), conv1size 15.  No pass mark.

Per width: `--warmup` (5) untimed and `--steps` (>= 20) timed calls between two device events -> ms per call, for
    feature_call          both losses, both data gradients, head gradients included
    head_grad_call        `delta_head_grad` alone on the same pairs in the same process: what the library could do before; the
                          difference is the cost of the feature
    torch_autograd        the same two losses and d / d l, d / d r by torch autograd in float32 on the same GPU, with the difference
                          tensor |l - r| materialised (66 MB per pair at 360 columns)
then `--profiled` (5) calls of each library entry under profile_begin / profile_end -> mean ms per kernel class:
    yaw_kernels_ms        correlation forward, yaw loss, both correlation gradients (class corr_head)
    delta_data_grad_ms    the two MFMA walks (class delta_prep of the feature call minus that of the head-gradient call, which holds
                          the c_conv1 weight gradient gw1_mfma_kernel); delta_data_gflop counts both walks (each forms E once)
    gw1_ms                the c_conv1 weight gradient + bias of the head-gradient call, gw1_gflop its contraction
Output: ONE JSON object, written to --out (profiles/feature_grad.json) and to stdout.

    python tools/bench_feature_grad.py --steps 20 --warmup 5"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import synthetic as S  # noqa: E402
from tools.bench_head_train import WIDTHS, _stats, _timed  # noqa: E402


def _torch_losses(params, l, r, t, q, s, ov_scale, yaw_scale):
    """Both heads and both losses in torch float32, |l - r| materialised a pair at a time."""
    w1, b1, w2, b2, w3, b3, wd, bd = params
    n, W, _ = l.shape
    g = W // s
    R = g * s
    o1 = torch.stack([(torch.abs(l[p, :, None, :] - r[p, None, :R, :]).reshape(W, g, s * 128) @ w1.reshape(s * 128, 64)) + b1
                      for p in range(n)])
    x = o1[:, :R].reshape(n, g, s, g, 64).permute(0, 1, 3, 2, 4).reshape(n, g, g, s * 64)
    o2 = torch.relu(x @ w2.reshape(s * 64, 128) + b2)
    o3 = torch.relu(torch.nn.functional.conv2d(o2.permute(0, 3, 1, 2), w3.permute(3, 2, 0, 1), b3))
    y = torch.sigmoid(o3.permute(0, 2, 3, 1).reshape(n, -1) @ wd.reshape(-1) + bd.reshape(()))
    lov = (ov_scale / n) * torch.sigmoid(24.0 * torch.abs(y - t) - 6.0).sum()
    m = torch.einsum("nic,njc->nij", l, r)
    jj = torch.arange(W, device=l.device)
    idx = (jj[:, None] + jj[None, :] + W // 2) % W
    z = m[:, idx, jj[None, :]].sum(dim=2)
    ce = (1.0 - q) * z + (1.0 + (W - 1.0) * q) * (torch.log1p(torch.exp(-torch.abs(z))) + torch.relu(-z))
    return lov + (yaw_scale / (n * W)) * ce.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profiled", type=int, default=5)
    ap.add_argument("--widths", type=int, nargs="*", default=sorted(WIDTHS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_grad.json"))
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        ap.error("at least 5 warm-up and 20 timed calls")
    from overlapnet_amd.engine import OvnEngine
    out = {"pairs": a.pairs, "steps": a.steps, "warmup": a.warmup, "conv1size": 15, "device": torch.cuda.get_device_name(0), "widths": {}}
    for fw in a.widths:
        h, w, a3 = WIDTHS[fw]
        cfg = dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=fw, additional_unsymmetric_layer3a=a3)
        weights = S.make_test_weights(4, seed=0, model_cfg=cfg, feat_w=fw)
        eng = OvnEngine(h, w, 4)
        try:
            eng.load_weights(weights, cfg)
            rng = np.random.default_rng(fw)
            # volumes scaled so that the correlation logits are of order one (as tests/_feature_grad_ref.py does)
            vols = torch.from_numpy((np.maximum(rng.normal(0.2, 1.0, size=(a.pairs + 1, fw, 128)), 0) / 64).astype(np.float32)).to(eng.device)
            lidx = list(range(a.pairs))
            ridx = [p + 1 for p in range(a.pairs)]
            targets = torch.from_numpy(rng.uniform(0, 1, a.pairs).astype(np.float32)).to(eng.device)
            bins = torch.from_numpy(rng.integers(0, fw, a.pairs).astype(np.int32)).to(eng.device)
            li, ri = eng._idx(lidx, a.pairs, a.pairs + 1), eng._idx(ridx, a.pairs, a.pairs + 1)

            def feature():
                return eng.heads_feature_grad(vols, vols, targets, bins, lidx=li, ridx=ri, want_head_grads=True)

            def head():
                return eng.delta_head_grad(vols, vols, targets, lidx=li, ridx=ri, scale=5.0)
            res = {"feature_call": _stats(_timed(feature, a.warmup, a.steps)), "head_grad_call": _stats(_timed(head, a.warmup, a.steps))}
            res["feature_cost_ms"] = res["feature_call"]["mean_ms"] - res["head_grad_call"]["mean_ms"]
            prof = {"feature": [], "head": []}
            for _ in range(a.profiled):
                for name, fn in (("feature", feature), ("head", head)):
                    eng.profile_begin()
                    fn()
                    prof[name].append(eng.profile_end())
            mean = lambda name, kind: float(np.mean([p[kind][0] for p in prof[name]]))      # noqa: E731
            res["yaw_kernels_ms"] = mean("feature", "corr_head")
            res["gw1_ms"] = mean("head", "delta_prep")
            res["delta_data_grad_ms"] = mean("feature", "delta_prep") - res["gw1_ms"]
            g = fw // 15
            res["gw1_gflop"] = 2.0 * a.pairs * (128 * 15) * (15 * g * g) * 64 / 1e9
            res["delta_data_gflop"] = 2 * 2.0 * a.pairs * (15 * g) ** 2 * 128 * 64 / 1e9
            res["yaw_gflop"] = 3 * 2.0 * a.pairs * fw * fw * 128 / 1e9
            params = [torch.from_numpy(np.asarray(weights[k], np.float32)).to(eng.device) for k in eng.HEAD_PARAMS]
            l, r = vols[lidx].clone().requires_grad_(True), vols[ridx].clone().requires_grad_(True)
            q = torch.zeros((a.pairs, fw), device=eng.device)
            q[torch.arange(a.pairs, device=eng.device), bins.long()] = (targets > 0.7).float()

            def autograd():
                torch.autograd.grad(_torch_losses(params, l, r, targets, q, 15, 5.0, 1.0), [l, r])
            res["torch_autograd"] = _stats(_timed(autograd, a.warmup, a.steps))
            out["widths"][str(fw)] = res
        finally:
            eng.close()
    text = json.dumps(out, sort_keys=True, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
