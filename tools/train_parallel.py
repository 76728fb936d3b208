"""Train the whole network on every GPU of a node (`train.DataParallelTrainer`):

    python tools/train_parallel.py --gpus 8 --config network.yml --npz train_set.npz [more.npz ...] \\
        --epochs 100 --batch-size 64 --out model.npz [--lr 1e-3 --lr-alpha 0.99 --seed 0 --frozen-legs] [--rehearsal]

The program starts one rank per GPU itself, each a fresh child process of this one (nccl = RCCL, one device per rank, rendezvous on
127.0.0.1); no process ever replaces its program.  --config is the network.yml the reference reads (YAML, or the same keys as
JSON); its `pretrained_weightsfilename` gives the start weights (none: the seeded random initialisation, identical on every rank).
--batch-size is the GLOBAL batch.  Rank 0 writes --out (a file `pretrained_weightsfilename` loads) and prints one JSON line.
--rehearsal puts all ranks on ONE GPU with gloo / host tensors in the collective: the same command path, no speed claim."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_RANKS = 16


def load_config(path):
    """network.yml as a dict: JSON text is taken as it is, anything else goes through PyYAML."""
    text = open(path).read()
    try:
        return json.loads(text)
    except ValueError:
        pass
    try:
        import yaml
    except ImportError:
        raise SystemExit("%s is not JSON and PyYAML is not installed" % path)
    return yaml.safe_load(text)


def free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(args, argv):
    """One child per rank; the first failure ends the others.  Returns the exit code."""
    port = int(os.environ.get("MASTER_PORT", "0")) or free_port()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # RCCL across processes: dmabuf IPC
        env.setdefault("OMP_NUM_THREADS", str(max(1, 16 // args.gpus)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    try:
        left = list(procs)
        while left:
            for p in list(left):
                code = p.poll()
                if code is None:
                    continue
                left.remove(p)
                if code != 0 and rc == 0:
                    rc = code
                    for q in left:
                        q.terminate()
            if left:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


def run_rank(args):
    import torch
    import torch.distributed as dist
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import DataParallelTrainer
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    visible = torch.cuda.device_count()
    local = 0 if args.rehearsal else int(os.environ.get("LOCAL_RANK", rank))
    if visible < 1 or local >= visible:
        raise SystemExit("train_parallel: rank %d needs GPU %d, %d visible" % (rank, local, visible))
    torch.cuda.set_device(local)
    if world > 1:
        if args.rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    try:
        cfg = load_config(args.config)
        inf = Infer(cfg, device=local, seed=args.seed)
        try:
            tr = DataParallelTrainer(inf, args.lr, args.lr_alpha, train_legs=not args.frozen_legs)
            t0 = time.perf_counter()
            losses = tr.fit_from_npz(args.npz, args.epochs, args.batch_size, args.seed)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            if rank == 0:
                tr.save(args.out)
                out = {"tool": "tools/train_parallel.py", "world": world, "backend": "gloo" if args.rehearsal and world > 1 else
                       ("nccl" if world > 1 else "none"), "epochs": args.epochs, "steps": len(losses), "batch_size": args.batch_size,
                       "first_loss": losses[0], "last_loss": losses[-1], "seconds": round(seconds, 3), "out": args.out}
                if args.rehearsal:
                    out["rehearsal"] = True
                print(json.dumps(out), flush=True)
        finally:
            inf.close()
        if world > 1:
            dist.barrier()
    finally:
        if world > 1 and dist.is_initialized():
            dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--config", required=True)
    ap.add_argument("--npz", required=True, nargs="+", help="ground-truth files (tools/build_training_set.py writes them)")
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=None, help="GLOBAL batch (default: the config's batch_size)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--lr-alpha", type=float, default=0.99)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frozen-legs", action="store_true", help="train the head alone (the reference's 360OutputkLegsFixed)")
    ap.add_argument("--rehearsal", action="store_true", help="all ranks on ONE GPU, gloo: checks the command path, no speed claim")
    args = ap.parse_args()
    if not 1 <= args.gpus <= MAX_RANKS:
        ap.error("--gpus takes 1 .. %d" % MAX_RANKS)
    if "RANK" not in os.environ and args.gpus > 1:
        raise SystemExit(launch(args, sys.argv[1:]))
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", str(args.gpus))
    run_rank(args)


if __name__ == "__main__":
    main()
