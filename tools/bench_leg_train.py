"""Time of the leg's training path (`OvnEngine.leg_forward_train` / `leg_backward`, csrc/leg_backward.hip) and of the whole
`train.OverlapNetTrainer` step on `--scans` (32) scans of 64 x 900 x 4 with `additional_unsymmetric_layer3a`.  No pass mark; the aim
the record is judged against: leg forward + backward cost no more than the `heads_feature_grad` call on the pairs they feed.

`--warmup` (5) untimed and `--steps` (>= 20) timed calls between two device events -> ms per call, for
    leg_forward_train     the fp32 forward with every activation kept
    leg_backward          all 22 gradients; TFLOP/s over the FLOPs counted from the layer shapes (both gradients of every layer but the
                          first layer's data gradient, which is not computed)
    leg_f32               `engine.leg` under leg precision 'f32' on the same scans (the inference forward in the same arithmetic)
    heads_feature_grad    both losses on `--scans` / 2 pairs of those scans' feature volumes, head gradients included
    trainer_step          `OverlapNetTrainer.step` on the same pairs from cue files on disk: read, leg forward, heads, both row sums,
                          leg backward, Adagrad on 30 tensors, both re-registrations
    torch_autograd        the leg restated with float32 `F.conv2d` on the same GPU, forward + backward to the 22 tensors -- when
                          torch's convolution backward runs on this machine; otherwise the record says why not
then `--profiled` calls of leg_forward_train / leg_backward under profile_begin / profile_end -> ms of class leg_conv.
Output: ONE JSON object, written to --out (profiles/leg_train.json) and to stdout.  The per-kernel split of the backward comes
from running this tool under `rocprofv3 --kernel-trace --stats` in a run of its own (tools/summarize_leg_train_trace.py).

    python tools/bench_leg_train.py --steps 20 --warmup 5"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from overlapnet_amd import weights as W  # noqa: E402
from tools import synthetic as S  # noqa: E402
from tools.bench_head_train import _stats, _timed  # noqa: E402

H, WI, C, FW = 64, 900, 4, 360


def leg_flops(layers, h, w):
    """-> (forward FLOPs per scan, backward FLOPs per scan): 2 K cout per output pixel per GEMM; the backward has the weight gradient
    of every layer and the data gradient of every layer but the first."""
    fwd = bwd = 0.0
    for li, l in enumerate(layers):
        h, w = (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1
        f = 2.0 * l.kh * l.kw * l.cin * l.cout * h * w
        fwd += f
        bwd += f * (2 if li else 1)
    return fwd, bwd


def _torch_leg(params, layers, x):
    for li, l in enumerate(layers):
        x = torch.relu(torch.nn.functional.conv2d(x, params[2 * li], params[2 * li + 1], stride=(l.sh, l.sw)))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profiled", type=int, default=3)
    ap.add_argument("--skip-trainer", action="store_true", help="leave out the trainer step (no files are written)")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leg_train.json"))
    a = ap.parse_args()
    if a.steps < 20 or a.warmup < 5:
        ap.error("at least 5 warm-up and 20 timed calls")
    if a.scans < 2 or a.scans % 2:
        ap.error("an even number of scans")
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapNetTrainer
    n, pairs = a.scans, a.scans // 2
    model = dict(S.REFERENCE_MODEL_CFG, inputShape=[H, WI], leg_output_width=FW, additional_unsymmetric_layer3a=True)
    layers = W.leg_layers(C, model)
    weights = S.make_test_weights(C, seed=0, model_cfg=model, feat_w=FW)
    fwd_flop, bwd_flop = leg_flops(layers, H, WI)
    out = {"scans": n, "pairs": pairs, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "input": [H, WI, C], "leg_forward_gflop_per_scan": fwd_flop / 1e9, "leg_backward_gflop_per_scan": bwd_flop / 1e9}
    rng = np.random.default_rng(0)
    images = rng.uniform(-1.0, 1.0, (n, H, WI, C)).astype(np.float32)
    images[..., 0] = rng.uniform(0.0, 1.0, (n, H, WI)).astype(np.float32)
    with tempfile.TemporaryDirectory() as root:
        names = ["%06d" % i for i in range(n)]
        if not a.skip_trainer:
            for sub in ("depth", "normal"):
                os.makedirs(os.path.join(root, "07", sub))
            for i, name in enumerate(names):
                np.save(os.path.join(root, "07", "depth", name + ".npy"), np.ascontiguousarray(images[i, :, :, 0]))
                np.save(os.path.join(root, "07", "normal", name + ".npy"), np.ascontiguousarray(images[i, :, :, 1:4]))
        cfg = {"model": model, "infer_seqs": "07", "data_root_folder": root, "use_depth": True, "use_normals": True,
               "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": n,
               "pretrained_weightsfilename": "", "precision": "f32", "stream_ahead": False}
        inf = Infer(cfg, weights=weights)
        try:
            eng = inf.engine
            x = torch.from_numpy(images).to(eng.device)
            acts = eng.leg_forward_train(x)
            feats = acts[-1].view(n, FW, 128)
            # d L / d feats of the right magnitude: the heads' own, on pairs (2 p, 2 p + 1); volumes scaled so that the logits are O(1)
            scale = float(1.0 / max(1e-6, float(feats.abs().max()) * 8.0))
            vols = (feats * scale).contiguous()
            lidx, ridx = list(range(0, n, 2)), list(range(1, n, 2))
            targets = rng.uniform(0, 1, pairs).astype(np.float32)
            bins = rng.integers(0, FW, pairs).astype(np.int32)
            li, ri = eng._idx(lidx, pairs, n), eng._idx(ridx, pairs, n)
            tt, bt = torch.from_numpy(targets).to(eng.device), torch.from_numpy(bins).to(eng.device)

            def heads():
                return eng.heads_feature_grad(vols, vols, tt, bt, lidx=li, ridx=ri, want_head_grads=True, want_corr=False)
            r = heads()
            from overlapnet_amd.train import sum_rows_by_entry
            dfeat = (sum_rows_by_entry(r["dfeat_l"], lidx, n) + sum_rows_by_entry(r["dfeat_r"], ridx, n)).contiguous()

            def forward():
                return eng.leg_forward_train(x)

            def backward():
                return eng.leg_backward(x, acts, dfeat)

            def leg_f32():
                return eng.leg(x)
            out["leg_forward_train"] = _stats(_timed(forward, a.warmup, a.steps))
            out["leg_backward"] = _stats(_timed(backward, a.warmup, a.steps))
            out["leg_backward"]["tflops"] = bwd_flop * n / (out["leg_backward"]["mean_ms"] * 1e-3) / 1e12
            out["leg_forward_train"]["tflops"] = fwd_flop * n / (out["leg_forward_train"]["mean_ms"] * 1e-3) / 1e12
            out["leg_f32"] = _stats(_timed(leg_f32, a.warmup, a.steps))
            out["heads_feature_grad"] = _stats(_timed(heads, a.warmup, a.steps))
            out["leg_forward_plus_backward_ms"] = out["leg_forward_train"]["mean_ms"] + out["leg_backward"]["mean_ms"]
            out["aim_met"] = bool(out["leg_forward_plus_backward_ms"] <= out["heads_feature_grad"]["mean_ms"])
            out["workspace_mb"] = eng.workspace_bytes() / 2.0 ** 20
            prof = {"forward": [], "backward": []}
            for _ in range(a.profiled):
                for name, fn in (("forward", forward), ("backward", backward)):
                    eng.profile_begin()
                    fn()
                    prof[name].append(eng.profile_end()["leg_conv"][0])
            out["leg_conv_class_ms"] = {k: float(np.mean(v)) for k, v in prof.items()}
            if not a.skip_trainer:
                tr = OverlapNetTrainer(inf, 1e-5)
                ln, rn = [names[i] for i in lidx], [names[i] for i in ridx]
                out["trainer_step"] = _stats(_timed(lambda: tr.step(ln, rn, targets, bins), a.warmup, a.steps))
            if not a.skip_torch:
                try:
                    params = []
                    for l in layers:
                        params.append(torch.from_numpy(np.ascontiguousarray(weights[l.name + "/kernel"].transpose(3, 2, 0, 1)))
                                      .to(eng.device).requires_grad_(True))
                        params.append(torch.from_numpy(weights[l.name + "/bias"]).to(eng.device).requires_grad_(True))
                    xn = x.permute(0, 3, 1, 2).contiguous()
                    dn = dfeat.view(n, 1, FW, 128).permute(0, 3, 1, 2).contiguous()

                    def autograd():
                        torch.autograd.grad((_torch_leg(params, layers, xn) * dn).sum(), params)
                    out["torch_autograd"] = _stats(_timed(autograd, a.warmup, a.steps))
                except Exception as e:                      # torch's convolution backward does not run on this machine
                    out["torch_autograd"] = {"not_measured": "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])}
        finally:
            inf.close()
    text = json.dumps(out, sort_keys=True, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
