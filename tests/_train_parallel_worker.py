"""Worker of tests/test_gpu_train_parallel.py: one of WORLD_SIZE processes that share cuda:0 (gloo rendezvous on 127.0.0.1, host
tensors in the collective) and train the fixture of tests/_leg_grad_ref.py with `train.DataParallelTrainer`.  argv: <work dir>
(the cue files lie under <work dir>/data).  Every rank writes <work dir>/rank<r>.json; rank 0 also writes grads.npz (the reduced
gradients of the global batch) and trained.npz."""
import hashlib
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _head_grad_ref as R  # noqa: E402
from tests import _leg_grad_ref as L  # noqa: E402


def infer_cfg(root, weights_file="", **model_extra):
    t = L.TRAINER
    return {"model": dict(R.model_cfg(t["W"], t["s"]), **model_extra), "infer_seqs": "07", "data_root_folder": str(root),
            "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
            "use_intensity": False, "batch_size": 8, "pretrained_weightsfilename": weights_file, "precision": "f32",
            "stream_ahead": False}


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).tobytes())
    return h.hexdigest()


def state(tr):
    return digest(tr.flat_params, tr.flat_accum)


def main():
    from overlapnet_amd._lib import OvnError
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import DataParallelTrainer
    work = sys.argv[1]
    root = os.path.join(work, "data")
    torch.cuda.set_device(0)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {"rank": rank, "world": world}
    try:
        t, x = L.TRAINER, L.trainer_inputs()
        names = ["%06d" % i for i in range(x["images"].shape[0])]
        batch = ([names[i] for i in x["left"]], [names[i] for i in x["right"]], x["targets"], x["bins"])

        def fresh(**kw):
            inf = Infer(infer_cfg(root, **{k: v for k, v in kw.items() if k != "train_legs"}), weights=x["weights"])
            return inf, DataParallelTrainer(inf, t["lr"], t["alpha"], t["loss"], train_legs=kw.get("train_legs", True))

        # 1. gradients of the global batch (pairs 3 / 3 / 2)
        inf, tr = fresh()
        try:
            out["shares"] = [tr.world, tr.rank, tr.count]
            g = tr.gradients(*batch)
            out["grad_digest"] = digest(*[g[n] for n in tr.names], g["loss_overlap"], g["loss_yaw"])
            out["grad_losses"] = [float(g["loss_overlap"]), float(g["loss_yaw"])]
            if rank == 0:
                np.savez(os.path.join(work, "grads.npz"), **{n.replace("/", "__"): g[n].cpu().numpy() for n in tr.names})
        finally:
            inf.close()

        # 2. four steps on the fixed batch, twice from scratch: the same bits on every rank, after every step, on both runs
        out["runs"] = []
        for run in range(2):
            inf, tr = fresh()
            try:
                inf.feature_volumes = [np.zeros((1, t["W"], 128), np.float32)]
                losses, states = [], []
                for _ in range(t["steps"]):
                    losses.append(tr.step(*batch))
                    states.append(state(tr))
                g = tr.gradients(*batch)
                losses.append(float(g["loss_overlap"] + g["loss_yaw"]))
                post = bool(len(inf.feature_volumes) == 0 and inf._qa is None and all(
                    np.array_equal(np.asarray(inf._weights[n]).reshape(-1), p.cpu().numpy().reshape(-1)) for n, p in zip(tr.names, tr.params)))
                out["runs"].append({"losses": losses, "states": states, "post_conditions": post})
                if run == 0 and rank == 0:
                    tr.save(os.path.join(work, "trained.npz"))
            finally:
                inf.close()

        # 3. fit, one epoch at batch_size 3: batches of 3, 3 and 2 pairs -> shares 1/1/1, 1/1/1 and 1/1/0 (rank 2 idle)
        inf, tr = fresh()
        try:
            fit_losses = tr.fit(*batch, epochs=1, batch_size=3)
            out["fit"] = {"losses": fit_losses, "state": state(tr), "epoch": tr.epoch, "idle_last": bool(tr.last is None),
                          "cache_empty": bool(len(inf.feature_volumes) == 0)}

            # 4. one rank fails: scan 4 occurs only in rank 1's pairs; its depth image disappears, every rank raises, nothing moves,
            #    and the repaired step succeeds
            before = state(tr)
            cue = os.path.join(root, "07", "depth", names[4] + ".npy")
            dist.barrier()
            if rank == 1:
                os.rename(cue, cue + ".away")
            dist.barrier()
            try:
                tr.step(*batch)
                out["failure"] = {"raised": False}
            except OvnError as e:
                out["failure"] = {"raised": True, "message": str(e), "unchanged": bool(state(tr) == before)}
            dist.barrier()
            if rank == 1:
                os.rename(cue + ".away", cue)
            dist.barrier()
            loss = tr.step(*batch)
            out["failure"]["repaired_loss"] = loss
            out["failure"]["repaired_moved"] = bool(state(tr) != before)
            out["failure"]["repaired_state"] = state(tr)
        finally:
            inf.close()

        # 5. frozen legs under deltaLayer_negateDiffs: only the head part travels
        inf, tr = fresh(deltaLayer_negateDiffs=True, train_legs=False)
        try:
            g = tr.gradients(*batch)
            tr.step(*batch)
            after = tr.weights()
            step = after["c_conv1/kernel"] - x["weights"]["c_conv1/kernel"]
            gf = g["c_conv1/kernel"].cpu().numpy()
            moved = step != 0
            out["frozen"] = {"keys": sorted(g), "count": tr.count, "state": state(tr),
                             "legs_untouched": bool(all(np.array_equal(after[k], x["weights"][k]) for k in L.leg_names(4, x["cfg"]))),
                             "moved_fraction": float(moved.mean()),
                             "against_gradient": bool(np.all(np.sign(step[moved]) == -np.sign(gf[moved])))}
        finally:
            inf.close()
        json.dump(out, open(os.path.join(work, "rank%d.json" % rank), "w"))
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
