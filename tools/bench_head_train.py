"""Time of one gradient call of the head-fitting path (`OvnEngine.delta_head_grad` -> ovn_delta_head_grad, csrc/delta_head_backward.hip)
on 16 pairs at feature widths 360 (64 x 900) and 371 (32 x 900), conv1size 15.

Per width: `--warmup` (5) untimed and `--steps` (>= 20) timed calls between two device events -> ms per call (mean and spread over
the timed calls); then one call under profile_begin / profile_end -> ms per kernel class (forward, loss + Dense gradients, c_conv3 /
c_conv2 / c_conv1 gradients).  Two comparison figures from the same process, neither a pass mark:
    forward_c12_fp32_ms   the fused fp32 MFMA kernel of the inference path (DeltaLayer + c_conv1 + c_conv2, head precision 'f32') on
                          the same pairs: its c_conv1 contraction does the FLOPs of the gW1 kernel
    torch_autograd_ms     the same loss and gradients by torch autograd in float32 on the same GPU, with the difference tensor
                          materialised as the reference's DeltaLayer does (generateNet.py:45-59)
Output: ONE JSON object on stdout.

    python tools/bench_head_train.py --steps 20 --warmup 5 > profiles/head_train.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import synthetic as S  # noqa: E402

WIDTHS = {360: (64, 900, True), 371: (32, 900, False)}
GRAD_CLASSES = {"forward": "delta_c12", "loss_dense": "dense_sigmoid", "c_conv3": "c_conv3", "c_conv2": "delta_c2", "c_conv1": "delta_prep"}


def _timed(fn, warmup, steps):
    """ms of every one of `steps` calls of fn (device events), after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def _stats(ms):
    return {"mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "calls": len(ms)}


def _torch_loss(params, l, r, t, s, scale):
    """The Delta head and the reference's sigmoid loss in torch, |l - r| materialised (one pair at a time: (W, R, 128) floats)."""
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
    return (scale / n) * torch.sigmoid(24.0 * torch.abs(y - t) - 6.0).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--widths", type=int, nargs="*", default=sorted(WIDTHS))
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
            vols = torch.from_numpy(np.maximum(rng.normal(0.2, 1.0, size=(a.pairs + 1, fw, 128)), 0).astype(np.float32)).to(eng.device)
            lidx = list(range(a.pairs))
            ridx = [p + 1 for p in range(a.pairs)]
            targets = torch.from_numpy(rng.uniform(0, 1, a.pairs).astype(np.float32)).to(eng.device)
            li, ri = eng._idx(lidx, a.pairs, a.pairs + 1), eng._idx(ridx, a.pairs, a.pairs + 1)
            res = {"grad_call": _stats(_timed(lambda: eng.delta_head_grad(vols, vols, targets, lidx=li, ridx=ri, scale=5.0),
                                              a.warmup, a.steps))}
            eng.profile_begin()
            eng.delta_head_grad(vols, vols, targets, lidx=li, ridx=ri, scale=5.0)
            prof = eng.profile_end()
            res["grad_kernels_ms"] = {name: prof[kind][0] for name, kind in GRAD_CLASSES.items()}
            g = fw // 15
            res["gw1_gflop"] = 2.0 * a.pairs * (128 * 15) * (15 * g * g) * 64 / 1e9
            eng.set_head_precision("f32")
            _timed(lambda: eng.heads(vols, vols, lidx=li, ridx=ri), a.warmup, 1)
            ms = []
            for _ in range(a.steps):
                eng.profile_begin()
                eng.heads(vols, vols, lidx=li, ridx=ri)
                ms.append(eng.profile_end()["delta_c12"][0])
            res["forward_c12_fp32_ms"] = _stats(ms)
            params = [torch.from_numpy(np.asarray(weights[k], np.float32)).to(eng.device).requires_grad_(True) for k in eng.HEAD_PARAMS]
            l, r = vols[lidx], vols[ridx]

            def autograd():
                torch.autograd.grad(_torch_loss(params, l, r, targets, 15, 5.0), params)
            res["torch_autograd_ms"] = _stats(_timed(autograd, a.warmup, a.steps))
            out["widths"][str(fw)] = res
        finally:
            eng.close()
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
