"""Batched loop-closure queries (`OvnEngine.heads_segments` + `top_k_segments`, k = 1) against the two older ways of running the
same queries, in one process, f16x3 at W = 360 with spectra and Delta cache rows (what `Infer` caches):
  loop     the per-query chain: `heads` 1-vs-N + `best_match` on the device + the record's copy to the host, per query;
  indexed  the existing indexed route on the concatenated pairs (`heads` with lidx / ridx) + every score to the host;
  batch    ONE `heads_segments` + ONE `top_k_segments` + ONE copy of the B records.
Workloads: (1) the 83 non-empty gated lists of the demo3 transcript (tests/golden/demo_transcript.json; its frame ids index a
synthetic 259-frame pool), (2) 256 segments x 100 candidates, (3) 8 segments x 1024 candidates.  Each step of each way is timed
with HIP events around the whole step (host work included), `--warmup` untimed steps first; the ways alternate step by step and
the reported time is the median over `--steps` steps.  `k_walk_frac`: the batch's pair-weighted K walk of the Delta contraction
(`head_walk_stats` of each segment's 1-vs-N sweep: the segmented pass walks each pair as that sweep does).
Output: ONE JSON object on stdout.

    python tools/bench_batch_queries.py > profiles/batch_queries.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _volumes(rng, k):
    """Leg-output-like volumes: ReLU of a shifted normal, 32 dead channels each (what compaction drops)."""
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, 360, 128)), 0).astype(np.float32)
    for i in range(k):
        v[i][:, rng.permutation(128)[:32]] = 0
    return v


def _transcript_lists():
    with open(os.path.join(ROOT, "tests", "golden", "demo_transcript.json")) as f:
        d = json.load(f)
    calls = [(int(c["cur"]), [int(r) for r in c["refs"]]) for c in d["demo3"] if c.get("event") == "infer_multiple"]
    return [(cur, refs) for cur, refs in calls if refs]


def _workloads(rng):
    w1 = _transcript_lists()
    w2 = [(int(q), rng.integers(0, 1024, 100).tolist()) for q in rng.integers(0, 1024, 256)]
    w3 = [(int(q), rng.permutation(1024).tolist()) for q in rng.integers(0, 1024, 8)]
    return {"demo3_gated_lists": (259, w1), "256x100": (1024, w2), "8x1024": (1024, w3)}


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    assert a.steps >= 10
    from tools import synthetic as S
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    eng = OvnEngine(64, 900, 4, device=0)
    eng.load_weights(S.make_trained_like_weights(4), S.REFERENCE_MODEL_CFG)
    rng = np.random.default_rng(0)
    pool = torch.from_numpy(_volumes(rng, 1024)).cuda()
    spec, dc = eng.spectrum(pool), eng.delta_cache(pool)
    res = {"device": torch.cuda.get_device_name(0), "head_precision": eng.head_precision, "steps": a.steps, "warmup": a.warmup,
           "head_chunk": eng.head_pipeline()[0], "workloads": {}}
    for name, (npool, segs) in _workloads(rng).items():
        fv, sp, dcp = pool[:npool], spec[:npool], dc[:npool]
        q = np.array([s[0] for s in segs], np.int32)
        lists = [np.array(s[1], np.int32) for s in segs]
        offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
        cand_h = np.concatenate(lists)
        cand = torch.from_numpy(cand_h).cuda()
        ridx = torch.from_numpy(np.repeat(q, np.diff(offs)).astype(np.int32)).cuda()
        seg_c = [cand[int(offs[b]):int(offs[b + 1])] for b in range(len(q))]
        n = int(offs[-1])

        def loop():
            out = []
            for b in range(len(q)):
                qi = int(q[b])
                r = eng.heads(fv, fv[qi:qi + 1], lidx=seg_c[b], spec_l=sp, spec_r=sp[qi:qi + 1], dcache_l=dcp)
                out.append(eng.best_match(r["overlap"], r["yaw"], 0.3, ids=seg_c[b]).cpu())
            return out

        def indexed():
            r = eng.heads(fv, fv, lidx=cand, ridx=ridx, spec_l=sp, spec_r=sp)
            return torch.stack([r["overlap"].view(torch.int32), r["yaw"]]).cpu()

        def batch():
            r = eng.heads_segments(fv, fv, cand, q, offs, spec_pool=sp, spec_q=sp, dcache_pool=dcp)
            return eng.top_k_segments(r["overlap"], offs, r["yaw"], 1, 0.3, ids=cand).cpu()

        # the three ways agree (the batch's records are the loop's, bit for bit)
        want = torch.stack(loop())
        assert torch.equal(batch()[:, 0], want), name
        ts = {"loop": [], "indexed": [], "batch": []}
        for f in (loop, indexed, batch):
            _median_ms(f, 0, a.warmup)
        for _ in range(a.steps):      # alternate the ways step by step
            for key, f in (("loop", loop), ("indexed", indexed), ("batch", batch)):
                ts[key] += _median_ms(f, 1, 0)
        row = {"segments": len(q), "pairs": n}
        for key, t in ts.items():
            ms = float(np.median(t))
            row[key] = {"ms_per_call": round(ms, 4), "pairs_per_s": round(n / (ms * 1e-3), 1)}
        row["batch_vs_loop"] = round(row["loop"]["ms_per_call"] / row["batch"]["ms_per_call"], 3)
        row["batch_vs_indexed"] = round(row["indexed"]["ms_per_call"] / row["batch"]["ms_per_call"], 3)
        walked = 0.0
        for b in range(len(q)):
            qi = int(q[b])
            eng.heads(fv, fv[qi:qi + 1], lidx=seg_c[b], spec_l=sp, spec_r=sp[qi:qi + 1], dcache_l=dcp)
            walked += eng.head_walk_stats()["k_walk_frac"] * len(lists[b])
        row["k_walk_frac"] = round(walked / n, 4)
        res["workloads"][name] = row
        print(name, json.dumps(row), file=sys.stderr)
    eng.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
