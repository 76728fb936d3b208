"""GPU (MI355X): `train.DataParallelTrainer` on the trainer fixture of tests/_leg_grad_ref.py (W = 45, six
scans, eight pairs, precision f32).

World 3 -- three processes of tests/_train_parallel_worker.py on cuda:0 over gloo (the box has one GPU; with this process at most
four hold it), started ONCE for the module; pairs 3 / 3 / 2:
  - `gradients()` is bitwise identical on the three ranks, and on rank 0 every one of the 28 tensors lies within the project's own
    4 T of the fp64 whole network on the GLOBAL batch (`L.network_loss`, the GPU's leg and head masks forced in, taken from a
    single-process forward over all scans and pairs; T = the float32 CPU restatement's error, as test_gpu_leg_train.py); the global
    loss within 1e-3 relative of fp64.  With OVN_TRAIN_PARALLEL_PARITY_JSON set the ratios are written to that file;
  - four `step`s on the fixed batch: parameters and accumulators bitwise identical across ranks after every step; the loss sequence
    follows `L.trainer_losses64()` as closely as the single-process trainer's does (worst relative deviation <= 2 x the old one's,
    both printed); the last loss below the first; a second run gives the same bits;
  - `fit` with batch_size 3 (batches 3, 3, 2 -> shares 1/1/1 and 1/1/0) completes and the idle rank ends with the others' bits;
  - rank 1's cue file of one of ITS scans is missing: all three ranks raise, no parameter moved, the repaired step succeeds;
  - train_legs=False with deltaLayer_negateDiffs: the leg tensors untouched on every rank, the file's c_conv1 kernel moves against
    the file's gradient.
World 1, in this process beside `OverlapNetTrainer`: `gradients()` bitwise equal; after one `step` from equal state
|dp| <= ulp(p) + 1e-5 lr per element (the update is at most lr in magnitude because a >= g^2; it comes from a handful of float32
operations that differ between torch's device arithmetic and the correctly rounded kernel by a few ulp each, under 1e-6 relative, and
1e-5 leaves a decade; one ulp of p covers the final subtraction); `save()` -> a fresh `Infer` reproduces `infer_one` bitwise.
tools/train_parallel.py --gpus 2 --rehearsal runs one epoch on the fixture and writes a file that loads as pretrained weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _head_grad_ref as R
from tests import _leg_grad_ref as L
from tests._train_parallel_worker import infer_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

_PARITY = {}


@pytest.fixture(scope="module")
def parity_file():
    yield
    path = os.environ.get("OVN_TRAIN_PARALLEL_PARITY_JSON")
    if path and _PARITY:
        with open(path, "w") as f:
            json.dump(_PARITY, f, indent=1, sort_keys=True)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _write_scans(base):
    """The trainer fixture's images as the cue files `Infer` reads (as the `scans` fixture of test_gpu_leg_train.py)."""
    x = L.trainer_inputs()
    seq = base / "data" / "07"
    for sub in ("depth", "normal"):
        os.makedirs(seq / sub)
    names = ["%06d" % i for i in range(x["images"].shape[0])]
    for i, name in enumerate(names):
        np.save(seq / "depth" / (name + ".npy"), np.ascontiguousarray(x["images"][i, :, :, 0]))
        np.save(seq / "normal" / (name + ".npy"), np.ascontiguousarray(x["images"][i, :, :, 1:4]))
    return base / "data", x, names


def _batch(x, names):
    return [names[i] for i in x["left"]], [names[i] for i in x["right"]], x["targets"], x["bins"]


@pytest.fixture(scope="module")
def scans(tmp_path_factory):
    return _write_scans(tmp_path_factory.mktemp("train_parallel"))


@pytest.fixture(scope="module")
def world3(scans):
    """The three ranks, run once: -> (work dir, [rank 0's, rank 1's, rank 2's report])."""
    root, _x, _names = scans
    work, world, port = str(root.parent), 3, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_train_parallel_worker.py"), work], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-3000:] for o in outs)
    return work, [json.load(open(os.path.join(work, "rank%d.json" % r))) for r in range(world)]


@pytest.fixture(scope="module")
def single(scans):
    """This process: the masks of a single-process forward over all scans and pairs, the fp64 / fp32 references with them, and the
    single-process trainer's four steps."""
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapNetTrainer
    root, x, names = scans
    t = L.TRAINER
    ln, rn, ov, yb = _batch(x, names)
    inf = Infer(infer_cfg(root), weights=x["weights"])
    try:
        xd = inf._inputs_device(names)
        acts = inf.engine.leg_forward_train(xd)
        feats = acts[-1].view(len(names), t["W"], 128)
        head = inf.engine.delta_head_grad(feats, feats, ov, lidx=x["left"], ridx=x["right"], loss=t["loss"], scale=5.0, want_activations=True)
        leg_masks = [(a > 0).cpu().numpy() for a in acts]
        head_masks = [(head["o2"] > 0).cpu().numpy(), (head["o3"] > 0).cpu().numpy()]
        tr = OverlapNetTrainer(inf, t["lr"], t["alpha"], t["loss"])
        losses = [tr.step(ln, rn, ov, yb) for _ in range(t["steps"])]
        g = tr.gradients(ln, rn, ov, yb)
        losses.append(float(g["loss_overlap"] + g["loss_yaw"]))
    finally:
        inf.close()
    refs = {dt: L.network_loss(x["weights"], x["images"], x["left"], x["right"], ov, yb, t["s"], x["cfg"], t["loss"], dtype=dt,
                               leg_masks=leg_masks, head_masks=head_masks) for dt in (torch.float64, torch.float32)}
    return {"refs": refs, "losses": losses}


def _worst_rel(losses, ref):
    return max(abs(a - b) / abs(b) for a, b in zip(losses, ref))


# ---- world 3 -------------------------------------------------------------------------------------------------------------------------

def test_world3_gradients_same_bits_and_within_4T_of_fp64(world3, single, parity_file):
    work, ranks = world3
    assert [r["shares"][:2] for r in ranks] == [[3, 0], [3, 1], [3, 2]]
    assert ranks[0]["grad_digest"] == ranks[1]["grad_digest"] == ranks[2]["grad_digest"]
    g = np.load(os.path.join(work, "grads.npz"))
    r32, r64 = single["refs"][torch.float32], single["refs"][torch.float64]
    names = list(R.HEAD_PARAMS) + L.leg_names(4, L.trainer_inputs()["cfg"])
    assert len(names) == 28 and sorted(g.files) == sorted(n.replace("/", "__") for n in names)
    ratios = {}
    for name in names:
        gpu = np.asarray(g[name.replace("/", "__")], np.float64)
        g64 = np.asarray(r64["grads"][name], np.float64)
        T = float(np.max(np.abs(np.asarray(r32["grads"][name], np.float64) - g64)))
        err = float(np.max(np.abs(gpu.reshape(g64.shape) - g64)))
        ratios[name] = err / T if T > 0 else (0.0 if err == 0 else float("inf"))
        print("world 3 %-22s T %.3e  gpu err %.3e  ratio %.3f" % (name, T, err, ratios[name]))
    _PARITY["world3_gradient_ratio_to_T"] = ratios
    _PARITY["world3_gradient_ratio_worst"] = max(ratios.values())
    for name in names:
        assert np.all(np.isfinite(g[name.replace("/", "__")])), name
        assert ratios[name] <= 4.0, (name, ratios[name])
    lov, lyaw = ranks[0]["grad_losses"]
    print("world 3 loss_overlap %.7f (fp64 %.7f)  loss_yaw %.7f (fp64 %.7f)" % (lov, r64["loss_overlap"], lyaw, r64["loss_yaw"]))
    assert abs(lov - r64["loss_overlap"]) <= 1e-3 * abs(r64["loss_overlap"]) + 1e-6
    assert abs(lyaw - r64["loss_yaw"]) <= 1e-3 * abs(r64["loss_yaw"]) + 1e-6
    assert abs((lov + lyaw) - (r64["loss_overlap"] + r64["loss_yaw"])) <= 1e-3 * abs(r64["loss_overlap"] + r64["loss_yaw"])


def test_world3_steps_same_bits_on_every_rank_and_run(world3, single, parity_file):
    _work, ranks = world3
    t = L.TRAINER
    first = ranks[0]["runs"][0]
    assert len(first["states"]) == t["steps"] and len(set(first["states"])) == t["steps"]          # every step moved the state
    for r in ranks:
        for run in r["runs"]:
            assert run["states"] == first["states"], (r["rank"], "states differ between ranks or runs")
            assert run["losses"] == first["losses"]
            assert run["post_conditions"], r["rank"]
    ref = L.trainer_losses64()
    new, old = _worst_rel(first["losses"], ref), _worst_rel(single["losses"], ref)
    for k, (a, b, c) in enumerate(zip(first["losses"], single["losses"], ref)):
        print("step %d  world 3 %.7f  single %.7f  fp64 %.7f" % (k, a, b, c))
    print("worst relative deviation from fp64: world 3 %.3e, single process %.3e" % (new, old))
    _PARITY["loss_worst_rel_dev_world3"], _PARITY["loss_worst_rel_dev_single"] = new, old
    assert new <= 2 * old, (new, old)
    assert first["losses"][-1] < first["losses"][0]


def test_world3_fit_with_an_idle_rank(world3):
    _work, ranks = world3
    fits = [r["fit"] for r in ranks]
    assert all(len(f["losses"]) == 3 and f["epoch"] == 1 and f["cache_empty"] for f in fits), fits
    assert fits[0]["losses"] == fits[1]["losses"] == fits[2]["losses"] and all(np.isfinite(fits[0]["losses"]))
    assert [f["idle_last"] for f in fits] == [False, False, True]               # the last batch has two pairs: rank 2 ran nothing
    assert fits[0]["state"] == fits[1]["state"] == fits[2]["state"]


def test_world3_one_rank_fails_all_raise_nothing_moves(world3):
    _work, ranks = world3
    for r in ranks:
        f = r["failure"]
        assert f["raised"] and "rank(s) [1]" in f["message"] and f["unchanged"], (r["rank"], f)
        assert f["repaired_moved"] and np.isfinite(f["repaired_loss"])
    assert "this rank" in ranks[1]["failure"]["message"] and "this rank" not in ranks[0]["failure"]["message"]
    assert ranks[0]["failure"]["repaired_state"] == ranks[1]["failure"]["repaired_state"] == ranks[2]["failure"]["repaired_state"]


def test_world3_frozen_legs_and_negated_differences(world3):
    _work, ranks = world3
    x = L.trainer_inputs()
    head = sum(int(np.prod(x["weights"][k].shape)) for k in R.HEAD_PARAMS)
    for r in ranks:
        f = r["frozen"]
        assert f["keys"] == sorted(list(R.HEAD_PARAMS) + ["loss_overlap", "loss_yaw"]) and f["count"] == head
        assert f["legs_untouched"] and f["moved_fraction"] > 0.5 and f["against_gradient"], (r["rank"], f)
    assert ranks[0]["frozen"]["state"] == ranks[1]["frozen"]["state"] == ranks[2]["frozen"]["state"]


# ---- world 1, beside the single-process trainer ------------------------------------------------------------------------------------------

def test_world1_equals_the_single_process_trainer(scans, parity_file):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import DataParallelTrainer, OverlapNetTrainer, lr_schedule
    root, x, names = scans
    t = L.TRAINER
    ln, rn, ov, yb = _batch(x, names)
    path = str(root / "trained_world1.npz")
    a, b = Infer(infer_cfg(root), weights=x["weights"]), Infer(infer_cfg(root), weights=x["weights"])
    try:
        old, new = OverlapNetTrainer(a, t["lr"], t["alpha"], t["loss"]), DataParallelTrainer(b, t["lr"], t["alpha"], t["loss"])
        assert new.world == 1 and new.names == old.names and new.count == sum(p.numel() for p in old.params)
        assert all(p.data_ptr() == new.flat_params.data_ptr() + 4 * off for p, off in
                   zip(new.params, np.concatenate([[0], np.cumsum([q.numel() for q in new.params])])))
        go, gn = old.gradients(ln, rn, ov, yb), new.gradients(ln, rn, ov, yb)
        for name in old.names:
            assert torch.equal(go[name].view(torch.int32), gn[name].view(torch.int32)), name
        assert float(gn["loss_overlap"]) == float(go["loss_overlap"]) and float(gn["loss_yaw"]) == float(go["loss_yaw"])
        lo, ln_ = old.step(ln, rn, ov, yb), new.step(ln, rn, ov, yb)
        assert abs(lo - ln_) <= 1e-6 * abs(lo)             # the two loss parts are added in float32 there, in float64 here
        lr = float(lr_schedule(0, t["lr"], t["alpha"]))
        worst = 0.0
        for name, p, q in zip(old.names, old.params, new.params):
            p, q = p.cpu().numpy().reshape(-1), q.cpu().numpy().reshape(-1)
            assert not np.array_equal(q, np.asarray(x["weights"][name], np.float32).reshape(-1)), name
            bound = np.spacing(np.abs(p)).astype(np.float64) + 1e-5 * lr
            d = np.abs(p.astype(np.float64) - q.astype(np.float64))
            worst = max(worst, float(np.max(d / bound)))
            assert np.all(d <= bound), (name, float(np.max(d / bound)))
        print("world 1: max |dp| / (ulp(p) + 1e-5 lr) against OverlapNetTrainer.step = %.3e" % worst)
        _PARITY["world1_step_max_dp_over_bound"] = worst
        assert len(b.feature_volumes) == 0 and b._qa is None
        new.save(path)
        mine = b.infer_one("000000.bin", "000001.bin")
    finally:
        a.close()
        b.close()
    fresh = Infer(infer_cfg(root, weights_file=path))
    try:
        theirs = fresh.infer_one("000000.bin", "000001.bin")
    finally:
        fresh.close()
    assert np.array_equal(np.asarray(mine[0]).view(np.uint32), np.asarray(theirs[0]).view(np.uint32))
    assert np.array_equal(mine[1], theirs[1])


# ---- the launcher ------------------------------------------------------------------------------------------------------------------

def test_launcher_rehearsal_writes_loadable_weights(scans):
    from overlapnet_amd import weights as WT
    from overlapnet_amd.infer import Infer
    root, x, names = scans
    work = root.parent / "launcher"
    os.makedirs(work)
    start, out = str(work / "start.npz"), str(work / "model.npz")
    WT.save_npz(start, x["weights"])
    json.dump(infer_cfg(root, weights_file=start), open(work / "network.yml", "w"))
    arr = np.stack([np.asarray(x["left"], np.float64), np.asarray(x["right"], np.float64), np.asarray(x["targets"], np.float64),
                    np.asarray(x["bins"], np.float64)], axis=1)
    np.savez(work / "train_set.npz", overlaps=arr, seq=np.full((len(arr), 2), "07"))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_parallel.py"), "--gpus", "2", "--rehearsal", "--config",
           str(work / "network.yml"), "--npz", str(work / "train_set.npz"), "--epochs", "1", "--batch-size", "4", "--lr", str(L.TRAINER["lr"]),
           "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["world"] == 2 and line["rehearsal"] is True and line["steps"] == 2 and line["backend"] == "gloo"
    trained = WT.load_npz(out)
    assert set(trained) == set(x["weights"])
    assert all(not np.array_equal(trained[k], x["weights"][k]) for k in R.HEAD_PARAMS)
    inf = Infer(infer_cfg(root, weights_file=out))
    try:
        ov, yaw = inf.infer_one("000000.bin", "000001.bin")
        assert np.all(np.isfinite(np.asarray(ov)))
    finally:
        inf.close()
