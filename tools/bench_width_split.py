"""The Delta head's two arithmetics at feature widths other than 360, side by side: the exact fp32 route (delta_head.hip) and the
split f16x3 route (delta_head_w_f16x3.hip, `OvnEngine.set_head_width_split(True)`), head precision 'f16x3' in both.

Per width in {371 (32 x 900), 422 (64 x 1024), 512 (32 x 1181)}: ONE engine, a 1-vs-N sweep (1 query vs --pool candidates) through
`engine.heads` on the volumes of tools/bench_width.py; the two routes alternate in rounds inside one process (clock and thermal
drift fall on both alike), per route and round `--warmup` untimed and `--steps` timed sweeps.  After the timed rounds one sweep per
route under profile_begin / profile_end gives the per-kind kernel ms.  Output: ONE JSON object on stdout with, per width and route,
pairs/s (median over rounds of the timed mean) and the kernel ms, plus the two figures the routes are compared by:
    contraction_ms      everything before c_conv3: delta_prep + delta_c12 + delta_c2
    contraction_ratio   split contraction_ms / exact delta_c12 ms   (the bar is <= 0.5 at 371 and 422)
    speedup             split pairs/s / exact pairs/s                (the bar is > 1 at every width)

    python tools/bench_width_split.py --rounds 3 --steps 10 --warmup 3"""
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
from tools.bench_width import _volumes  # noqa: E402

WIDTHS = {371: (32, 900, False), 422: (64, 1024, True), 512: (32, 1181, False)}
ROUTES = (("exact", False), ("split", True))
CONTRACTION = ("delta_prep", "delta_c12", "delta_c2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--widths", type=int, nargs="*", default=sorted(WIDTHS))
    a = ap.parse_args()
    from overlapnet_amd.engine import OvnEngine
    out = {"pool": a.pool, "rounds": a.rounds, "steps": a.steps, "head_precision": "f16x3", "widths": {}}
    for fw in a.widths:
        h, w, a3 = WIDTHS[fw]
        cfg = dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=fw, additional_unsymmetric_layer3a=a3)
        eng = OvnEngine(h, w, 4)
        try:
            eng.load_weights(S.make_test_weights(4, seed=0, model_cfg=cfg, feat_w=fw), cfg)
            eng.set_head_precision("f16x3")
            assert eng.feat_w == fw
            v = torch.from_numpy(_volumes(fw, a.pool + 1, fw)).to(eng.device)
            cands, q = v[:a.pool], v[a.pool:]
            rates = {name: [] for name, _ in ROUTES}
            for _ in range(a.rounds):
                for name, on in ROUTES:
                    eng.set_head_width_split(on)
                    for _ in range(a.warmup):
                        eng.heads(cands, q)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        eng.heads(cands, q)
                    torch.cuda.synchronize()
                    rates[name].append(a.pool * a.steps / (time.perf_counter() - t0))
            res = {}
            ov = {}
            for name, on in ROUTES:
                eng.set_head_width_split(on)
                eng.profile_begin()
                ov[name] = eng.heads(cands, q)["overlap"]
                prof = eng.profile_end()
                res[name] = {"pairs_per_s": float(np.median(rates[name])), "pairs_per_s_rounds": [float(x) for x in rates[name]],
                             "contraction_ms": float(sum(prof[k][0] for k in CONTRACTION)),
                             "kernels_ms": {k: round(x[0], 4) for k, x in prof.items() if x[1]}}
            res["contraction_ratio"] = res["split"]["contraction_ms"] / res["exact"]["kernels_ms"]["delta_c12"]
            res["speedup"] = res["split"]["pairs_per_s"] / res["exact"]["pairs_per_s"]
            res["max_abs_overlap_difference"] = float((ov["split"] - ov["exact"]).abs().max())
            out["widths"][str(fw)] = res
        finally:
            eng.close()
    out["bar"] = {"contraction_ratio_max_at_371_422": 0.5,
                  "met": all(out["widths"][str(fw)]["contraction_ratio"] <= 0.5 for fw in (371, 422) if str(fw) in out["widths"])
                  and all(r["speedup"] > 1 for r in out["widths"].values())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
