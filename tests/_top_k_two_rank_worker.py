"""Worker of tests/test_gpu_top_k_two_ranks.py: one of TWO processes that share cuda:0 (gloo rendezvous on 127.0.0.1, host tensors in
the collectives) and run `Infer(config, rank=, world=2).infer_top_k` on the references they own.  argv: <work dir>.  Rank 0 also
replays every call on the unsharded object and writes <work dir>/result.json."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import synthetic as S  # noqa: E402


def replay(work):
    """A streaming run with growing reference lists (all previous frames, gated windows, duplicates, empty lists), k cycling over
    {1, 5, 64} and the threshold over {0.3, None, 0.0}: every sharded list must equal the unsharded object's.  Then a failure of rank
    1's local work: both ranks raise, the frame does not count as fed, and the same frame fed again gives the unsharded list."""
    from overlapnet_amd.infer import Infer
    rank, world = dist.get_rank(), dist.get_world_size()
    cfg = json.load(open(os.path.join(work, "config.json")))
    frames = cfg.pop("_frames")
    w = S.make_test_weights(4, seed=0)
    sh = Infer(json.loads(json.dumps(cfg)), weights=w, rank=rank, world=world)
    ref = Infer(json.loads(json.dumps(cfg)), weights=w) if rank == 0 else None
    rng = np.random.default_rng(9)
    report = {"calls": 0, "nonempty": 0, "mismatch": [], "ks": []}
    for i in range(frames - 1):
        if i % 6 == 5:
            refs = []
        elif i % 4 == 3 and i > 8:
            refs = list(range(max(0, i - 12), i - 2))                          # a gated window of consecutive frames
        elif i % 5 == 2 and i > 3:
            refs = sorted(rng.choice(i, size=min(i, 6), replace=True).tolist())  # duplicates: equal scores, list order decides
        else:
            refs = list(range(i))
        k = (1, 5, 64)[i % 3]
        thr = (0.3, None, 0.0)[i % 3 if i % 2 else (i // 2) % 3]
        a = sh.infer_top_k(i, refs, k, thr)
        if rank == 0:
            b = ref.infer_top_k(i, refs, k, thr)
            report["ks"].append(k)
            report["nonempty"] += int(len(b) > 0)
            if a != b:
                report["mismatch"].append([i, k, thr, a, b])
        report["calls"] += 1
    # a failure of rank 1's local work reaches every rank; the frame is fed again after the repair
    i = frames - 1
    good_leg = sh._leg_device
    if rank == 1:
        def boom(names):
            raise Exception("Could not read depth image (simulated, rank 1 only)")
        sh._leg_device = boom
    sh._stream_ahead = False
    sh._drop_ahead()
    raised = [None, None]
    for j, refs in enumerate((list(range(i)), [])):
        try:
            sh.infer_top_k(i, refs, 5, 0.3)
            raised[j] = "returned"
        except Exception as ex:
            raised[j] = str(ex)[:80]
    both = [None, None]
    dist.all_gather_object(both, raised)
    report["one_rank_failure"] = both
    sh._leg_device = good_leg
    a = sh.infer_top_k(i, list(range(i)), 5, None)
    if rank == 0:
        report["retry_ok"] = a == ref.infer_top_k(i, list(range(i)), 5, None) and len(a) == 5
    stats = [None] * world
    dist.all_gather_object(stats, dict(sh.sharded_stats))
    report["stats"] = stats
    sh.close()
    if ref is not None:
        ref.close()
    return report


def main():
    work = sys.argv[1]
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
    try:
        out = replay(work)
        if dist.get_rank() == 0:
            json.dump(out, open(os.path.join(work, "result.json"), "w"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
