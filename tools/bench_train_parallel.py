"""Measurements behind DESIGN.md section 23 (data-parallel training) -> profiles/train_parallel.json.

  (a) kernel      `OvnEngine.grad_reduce_adagrad` alone at the real parameter count (all tensors of the 64 x 900 x 4 network with
                  `additional_unsymmetric_layer3a`), world 1, 2 and 8: device events around each of `--calls` (>= 200) calls after
                  `--warmup`; bytes from the shapes -- 4 world + 8 read, 8 written per element -> GB/s and the share of the HBM peak
                  (8.0 TB/s).  The calls rotate over enough buffer sets (> 512 MB together) that none is served from the 256 MB
                  Infinity Cache.  At this count a call lasts some 20 us, so launch and ramp weigh in; `kernel_16x_elements`
                  repeats worlds 1 and 8 on 16 x as many elements to show the streaming rate of the same code.
  (b) world1      `DataParallelTrainer.step` against `OverlapNetTrainer.step` (unchanged code) on the batch of
                  tools/bench_leg_train.py (32 scans, 16 pairs), alternated, three repetitions each of `--steps` timed steps.  The
                  new mean must not exceed the old mean by more than the larger of the two spreads (max - min of a trainer's three
                  repetition means): `"pass"`.
  (c) rehearsal   world 2 and 4, all ranks on ONE GPU over gloo (fresh child processes of this program): ms per step of the command
                  path, marked `"rehearsal": true` -- the ranks time-share one device, so there is no pairs/s claim.
A run on several GPUs over RCCL is a separate command, `tools/train_parallel.py --gpus N`; this tool does not make one.

    python tools/bench_train_parallel.py [--skip-rehearsal]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import synthetic as S  # noqa: E402
from tools.bench_head_train import _stats, _timed  # noqa: E402

H, WI, C, FW = 64, 900, 4, 360
HBM_PEAK_GBS = 8000.0
MODEL = dict(S.REFERENCE_MODEL_CFG, inputShape=[H, WI], leg_output_width=FW, additional_unsymmetric_layer3a=True)


def write_batch(root, n):
    """The batch of tools/bench_leg_train.py as cue files: n scans, pairs (2 p, 2 p + 1).  -> (left, right, targets, bins)."""
    rng = np.random.default_rng(0)
    images = rng.uniform(-1.0, 1.0, (n, H, WI, C)).astype(np.float32)
    images[..., 0] = rng.uniform(0.0, 1.0, (n, H, WI)).astype(np.float32)
    names = ["%06d" % i for i in range(n)]
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(root, "07", sub), exist_ok=True)
    for i, name in enumerate(names):
        np.save(os.path.join(root, "07", "depth", name + ".npy"), np.ascontiguousarray(images[i, :, :, 0]))
        np.save(os.path.join(root, "07", "normal", name + ".npy"), np.ascontiguousarray(images[i, :, :, 1:4]))
    targets = rng.uniform(0, 1, n // 2).astype(np.float32)
    bins = rng.integers(0, FW, n // 2).astype(np.int32)
    np.savez(os.path.join(root, "batch.npz"), targets=targets, bins=bins)
    return [names[i] for i in range(0, n, 2)], [names[i] for i in range(1, n, 2)], targets, bins


def config(root, n):
    return {"model": MODEL, "infer_seqs": "07", "data_root_folder": root, "use_depth": True, "use_normals": True,
            "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": n,
            "pretrained_weightsfilename": "", "precision": "f32", "stream_ahead": False}


def bench_kernel(eng, count, worlds, warmup, calls):
    out = {}
    dev = eng.device
    stride = (count + 3) // 4 * 4 + 4
    g = torch.Generator(device=dev).manual_seed(1)
    for world in worlds:
        per_call = count * (4 * world + 8) + count * 8
        sets = max(2, -(-(512 << 20) // per_call) + 1)
        bufs = [(torch.randn((world, stride), device=dev, generator=g) * 1e-3, torch.randn(count, device=dev, generator=g) * 0.1,
                 torch.zeros(count, device=dev)) for _ in range(sets)]
        w = [1.0 / world] * world
        k = [0]

        def call():
            rows, p, a = bufs[k[0] % sets]
            k[0] += 1
            eng.grad_reduce_adagrad(rows, w, p, a, 1e-5)
        ms = _timed(call, warmup, calls)
        st = _stats(ms)
        st["median_ms"] = float(np.median(ms))
        st.update({"world": world, "count": count, "bytes_read": count * (4 * world + 8), "bytes_written": count * 8, "buffer_sets": sets,
                   "gb_per_s": per_call / (st["mean_ms"] * 1e-3) / 1e9})
        st["share_of_hbm_peak"] = st["gb_per_s"] / HBM_PEAK_GBS
        out["world_%d" % world] = st
        del bufs
    return out


def bench_world1(root, n, warmup, steps, reps=3):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import DataParallelTrainer, OverlapNetTrainer
    ln, rn, targets, bins = write_batch(root, n)
    weights = S.make_test_weights(C, seed=0, model_cfg=MODEL, feat_w=FW)
    a, b = Infer(config(root, n), weights=weights), Infer(config(root, n), weights=weights)
    try:
        old, new = OverlapNetTrainer(a, 1e-5), DataParallelTrainer(b, 1e-5)
        count = new.count
        means = {"old": [], "new": []}
        for _ in range(reps):
            for key, tr in (("old", old), ("new", new)):
                means[key].append(float(np.mean(_timed(lambda: tr.step(ln, rn, targets, bins), warmup, steps))))
    finally:
        a.close()
        b.close()
    res = {k: {"repetition_means_ms": v, "mean_ms": float(np.mean(v)), "spread_ms": float(max(v) - min(v))} for k, v in means.items()}
    allowed = max(res["old"]["spread_ms"], res["new"]["spread_ms"])
    return count, {"scans": n, "pairs": n // 2, "steps_per_repetition": steps, "warmup": warmup, "repetitions": reps,
                   "overlapnet_trainer_step": res["old"], "data_parallel_trainer_step": res["new"],
                   "new_minus_old_ms": res["new"]["mean_ms"] - res["old"]["mean_ms"], "allowed_excess_ms": allowed,
                   "pass": bool(res["new"]["mean_ms"] - res["old"]["mean_ms"] <= allowed)}


def rehearsal_rank(root, n, warmup, steps, out_path):
    """One rank of (c): RANK / WORLD_SIZE / MASTER_* in the environment, every rank on cuda:0, gloo."""
    import torch.distributed as dist
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import DataParallelTrainer
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        names = ["%06d" % i for i in range(n)]
        ln, rn = [names[i] for i in range(0, n, 2)], [names[i] for i in range(1, n, 2)]
        with np.load(os.path.join(root, "batch.npz")) as z:      # written by the parent (write_batch)
            targets, bins = z["targets"], z["bins"]
        inf = Infer(config(root, n), weights=S.make_test_weights(C, seed=0, model_cfg=MODEL, feat_w=FW))
        try:
            tr = DataParallelTrainer(inf, 1e-5)
            st = _stats(_timed(lambda: tr.step(ln, rn, targets, bins), warmup, steps))
        finally:
            inf.close()
        if rank == 0:
            st.update({"world": world, "pairs": n // 2, "rehearsal": True, "backend": "gloo",
                       "note": "all ranks time-share ONE GPU and the gradients cross the host: the command path, not a scaling figure"})
            json.dump(st, open(out_path, "w"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def bench_rehearsal(root, n, world, warmup, steps):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out_path = os.path.join(root, "rehearsal_%d.json" % world)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rehearsal-rank", root, "--scans", str(n), "--warmup",
                                       str(warmup), "--steps", str(steps), "--rank-out", out_path], env=env))
    try:
        codes = [p.wait(timeout=900) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if any(codes):
        raise SystemExit("rehearsal at world %d failed: exit codes %s" % (world, codes))
    return json.load(open(out_path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rehearsal-steps", type=int, default=5)
    ap.add_argument("--skip-rehearsal", action="store_true")
    ap.add_argument("--rehearsal-rank", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--rank-out", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_parallel.json"))
    a = ap.parse_args()
    if a.rehearsal_rank:
        return rehearsal_rank(a.rehearsal_rank, a.scans, a.warmup, a.steps, a.rank_out)
    if a.calls < 200:
        ap.error("at least 200 timed kernel calls")
    if a.scans < 2 or a.scans % 2:
        ap.error("an even number of scans")
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GBS,
           "multi_gpu_rccl": "not measured (one GPU on the machine this ran on)"}
    with tempfile.TemporaryDirectory() as root:
        count, out["world1_step"] = bench_world1(root, a.scans, a.warmup, a.steps)
        from overlapnet_amd.engine import OvnEngine
        eng = OvnEngine(32, 247, 4)
        try:
            out["kernel"] = bench_kernel(eng, count, (1, 2, 8), 20, a.calls)
            # the same kernel on 16 x as many elements: its streaming rate, apart from the launch and ramp of a 20 us call
            out["kernel_16x_elements"] = bench_kernel(eng, 16 * count, (1, 8), 20, a.calls)
        finally:
            eng.close()
        if a.skip_rehearsal:
            out["rehearsal"] = "not measured"
        else:
            torch.cuda.synchronize()
            out["rehearsal"] = {"world_%d" % w: bench_rehearsal(root, a.scans, w, 2, a.rehearsal_steps) for w in (2, 4)}
    with open(a.out, "w") as f:
        f.write(json.dumps(out, sort_keys=True, indent=1) + "\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
