"""Heads throughput of the fp32 heads (delta_head.hip, corr_head.hip) across feature widths: a 1-vs-N sweep (1 query vs --pool
candidates) through `engine.heads` (the direct correlation head on the feature volumes, no spectra) at W = 360 in the fp32 head
mode (delta_c12_kernel<3,2>, corr_head_kernel<3,false>), at W = 371 (32 x 900, the leg's defaults: the same two instantiations) and
at W = 422 (64 x 1024, additional_unsymmetric_layer3a: <4,2> and <4,false>).  Seeded synthetic weights and ReLU-like random feature volumes (a quarter of the channels dead).

The widths alternate in rounds inside one process (clock and thermal drift fall on all of them alike); per width and round
`--warmup` untimed and `--steps` timed sweeps.  Output: ONE JSON object on stdout with pairs/s (median over rounds of the timed
mean), its ratio to the W = 360 fp32 rate, and the per-kernel ms of one sweep (profile_begin / profile_end): the Delta head
(contraction + c_conv3 + Dense) against the yaw head.

    python tools/bench_width.py --rounds 3 --steps 10 --warmup 3"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import synthetic as S  # noqa: E402

A3 = {"additional_unsymmetric_layer3a": True}
WIDTHS = {360: (64, 900, A3), 371: (32, 900, {}), 422: (64, 1024, A3)}


def _volumes(fw, k, seed):
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, fw, 128)), 0).astype(np.float32)
    v[:, :, rng.permutation(128)[:32]] = 0
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from overlapnet_amd.engine import OvnEngine
    state = {}
    for fw, (h, w, keys) in WIDTHS.items():
        cfg = dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=fw,
                   additional_unsymmetric_layer3a=bool(keys.get("additional_unsymmetric_layer3a", False)))
        eng = OvnEngine(h, w, 4)
        eng.load_weights(S.make_test_weights(4, seed=0, model_cfg=cfg, feat_w=fw), cfg)
        eng.set_head_precision("f32")
        assert eng.feat_w == fw
        v = torch.from_numpy(_volumes(fw, a.pool + 1, fw)).to(eng.device)
        state[fw] = (eng, v[:a.pool], v[a.pool:])
    rates = {fw: [] for fw in WIDTHS}
    for _ in range(a.rounds):
        for fw, (eng, cands, q) in state.items():
            for _ in range(a.warmup):
                eng.heads(cands, q)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                eng.heads(cands, q)
            torch.cuda.synchronize()
            rates[fw].append(a.pool * a.steps / (time.perf_counter() - t0))
    out = {"pool": a.pool, "rounds": a.rounds, "steps": a.steps, "head_precision": "f32", "widths": {}}
    base = float(np.median(rates[360]))
    for fw, (eng, cands, q) in state.items():
        eng.profile_begin()
        eng.heads(cands, q)
        prof = eng.profile_end()
        delta = sum(prof[k][0] for k in ("delta_c12", "c_conv3", "dense_sigmoid"))
        out["widths"][str(fw)] = {"pairs_per_s": float(np.median(rates[fw])), "vs_360_f32": float(np.median(rates[fw])) / base,
                                  "delta_ms": delta, "yaw_ms": prof["corr_head"][0],
                                  "kernels_ms": {k: round(v[0], 4) for k, v in prof.items() if v[1]}}
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
