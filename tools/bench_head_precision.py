"""Head arithmetic side by side on bench.py's headline workload: 1 query vs 1024 candidates, 64 x 900 x 4, seeded synthetic
(Glorot) weights and images, warm steps with QueryAhead (the next query's leg + spectrum on the side context), spectral yaw head.

Modes: f16x3 with the dead-channel compaction on and off, f32, bf16x3 (each with the leg arithmetic its parity gate uses: f16x3 leg
for f16x3, f32 leg for f32 and bf16x3).  The modes alternate in rounds inside one process (clock and thermal drift fall on all of
them alike); per mode and round `--warmup` untimed and `--steps` timed steps.  Output: ONE JSON object on stdout with pairs/s
(median over rounds of the timed mean), per-kernel ms per step (profile_begin / profile_end over one extra step), and max / p99
|d overlap| of the mode's results against tests/golden/parity_sweep_glorot.npz (fp64 oracle, same images and weights).

    python tools/bench_head_precision.py --rounds 3 --steps 20 --warmup 5 > profiles/<name>.json"""
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

MODES = [("f16x3", "f16x3", "f16x3", True), ("f16x3_nocompact", "f16x3", "f16x3", False), ("f32", "f32", "f32", True),
         ("bf16x3", "f32", "bf16x3", True)]   # (name, leg, head, compaction)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default=",".join(m[0] for m in MODES))
    a = ap.parse_args()
    from overlapnet_amd.engine import OvnEngine, QueryAhead
    C, POOL = 4, a.pool
    w = S.WEIGHT_SETS["glorot"](C)
    eng = OvnEngine(64, 900, C)
    eng.load_weights(w, S.REFERENCE_MODEL_CFG)
    dev = eng.device
    fx = S.load_fixture_images()
    pool_imgs = [(s, torch.from_numpy(imgs).to(dev)) for s, imgs in S.sweep_pool_images(POOL, C, 0, fx)]
    qimg = torch.from_numpy(S.sweep_query_image(C, fx)).to(dev)
    with np.load(os.path.join(ROOT, "tests", "golden", "parity_sweep_glorot.npz")) as z:
        gold = z["overlap"] if POOL == 1024 else None
    modes = [m for m in MODES if m[0] in a.modes.split(",")]
    state = {}
    for name, leg_p, head_p, compact in modes:   # candidates, their spectra and the query side per mode (leg arithmetic differs)
        eng.set_leg_precision(leg_p)
        eng.set_head_precision(head_p)
        eng.set_head_compaction(compact)
        cands = torch.empty((POOL, 360, 128), dtype=torch.float32, device=dev)
        for s, t in pool_imgs:
            eng.leg(t, out=cands[s:s + t.shape[0]])
        dc = eng.delta_cache(cands) if eng.has_delta_cache else None
        state[name] = (cands, eng.spectrum(cands), dc)
    qa = QueryAhead(eng, w, S.REFERENCE_MODEL_CFG)

    def set_mode(m):
        name, leg_p, head_p, compact = m
        eng.set_leg_precision(leg_p)
        eng.set_head_precision(head_p)
        eng.set_head_compaction(compact)

    def steps(m, k):
        cands, spec, dc = state[m[0]]
        r = None
        qa.submit(qimg)
        for i in range(k):
            if i + 1 < k:
                qa.submit(qimg)
            fv, sp = qa.take()
            r = eng.heads(cands, fv, spec_l=spec, spec_r=sp, dcache_l=dc)
        return r

    rates = {m[0]: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            set_mode(m)
            steps(m, a.warmup)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(m, a.steps)
            torch.cuda.synchronize()
            rates[m[0]].append(POOL * a.steps / (time.perf_counter() - t0))
    out = {"workload": "1 query vs %d candidates, 64x900x4, glorot weights, warm steps with QueryAhead, spectral yaw head" % POOL,
           "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "modes": {}}
    for m in modes:
        set_mode(m)
        steps(m, 2)
        torch.cuda.synchronize()
        eng.profile_begin()
        r = steps(m, 1)
        prof = eng.profile_end()
        ov = r["overlap"].cpu().numpy().astype(np.float64)
        rec = {"leg": m[1], "head": m[2], "compaction": m[3], "pairs_per_s": float(np.median(rates[m[0]])),
               "pairs_per_s_rounds": [float(x) for x in rates[m[0]]],
               "kernel_ms_per_step": {k: v[0] for k, v in prof.items() if v[1]}}
        if gold is not None:
            d = np.abs(ov - gold)
            rec["abs_d_overlap_vs_fp64"] = {"max": float(d.max()), "p99": float(np.percentile(d, 99))}
        out["modes"][m[0]] = rec
    if "bf16x3" in out["modes"] and "f32" in out["modes"]:
        out["bf16x3_over_f32"] = out["modes"]["bf16x3"]["pairs_per_s"] / out["modes"]["f32"]["pairs_per_s"]
    qa.close()
    eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
