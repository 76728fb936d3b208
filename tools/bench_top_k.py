"""`ovn_top_k` (csrc/top_k.hip) timed with HIP events next to `ovn_best_match` on the same scores: n in {1024, 1e5, 1e6} x
k in {1, 16, 256, 1024}, on overlap-like scores (uniform in [0, 1): few exponent bins, distinct values) and on heavy ties
(50 distinct values: the select walks the position digits too).  Per (data, n): `--warmup` untimed calls of each, then `--reps`
back-to-back calls of one kernel between two events, alternating top_k and best_match for `--rounds` rounds; the per-call time is
the median over the rounds.  Output: ONE JSON object on stdout.

    python tools/bench_top_k.py > profiles/top_k.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NS = (1024, 100000, 1000000)
KS = (1, 16, 256, 1024)


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    eng = OvnEngine(64, 900, 4, device=0)
    rng = np.random.default_rng(0)
    rows = []
    for data in ("uniform", "ties50"):
        for n in NS:
            v = rng.random(n) if data == "uniform" else rng.integers(0, 50, n) / 50.0
            ov = torch.from_numpy(v.astype(np.float32)).cuda()
            yaw = torch.from_numpy(rng.integers(-179, 181, n).astype(np.int32)).cuda()
            bm_out = torch.empty(4, dtype=torch.int32, device="cuda")
            outs = {k: torch.empty((k, 4), dtype=torch.int32, device="cuda") for k in KS}
            fns = {"best_match": lambda: eng.lib.ovn_best_match(eng._h, ov.data_ptr(), yaw.data_ptr(), None, n, 0.3, 0,
                                                                 bm_out.data_ptr(), eng._stream())}
            for k in KS:
                fns["top_k_%d" % k] = (lambda k=k: eng.lib.ovn_top_k(eng._h, ov.data_ptr(), yaw.data_ptr(), None, n, k, 0.3, 0,
                                                                     outs[k].data_ptr(), eng._stream()))
            for f in fns.values():       # the raw C calls (no Python wrapper in the timed loop); check the return codes once
                assert f() == 0
                for _ in range(a.warmup):
                    f()
            torch.cuda.synchronize()
            times = {name: [] for name in fns}
            for _ in range(a.rounds):
                for name, f in fns.items():
                    times[name].append(_time(f, a.reps))
            # the timed results are the real ones: k = 1 equals best_match's record
            assert torch.equal(outs[1].reshape(4), bm_out)
            bm = float(np.median(times["best_match"]))
            for k in KS:
                rows.append({"data": data, "n": n, "k": k, "top_k_ms": round(float(np.median(times["top_k_%d" % k])), 5),
                             "top_k_ms_min": round(float(np.min(times["top_k_%d" % k])), 5), "best_match_ms": round(bm, 5)})
    eng.close()
    worst_1e5 = max(r["top_k_ms"] for r in rows if r["n"] == 100000)
    print(json.dumps({"tool": "tools/bench_top_k.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
                      "method": "HIP events around reps back-to-back calls of the C entry point; median per-call time over rounds",
                      "target_ms_n1e5": 0.1, "worst_top_k_ms_n1e5": worst_1e5, "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
