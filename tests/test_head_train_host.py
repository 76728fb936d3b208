"""Host side of the head-fitting feature (no GPU): the torch restatement that the GPU gradients are measured against
(tests/_head_grad_ref.py) is pinned to the fp64 oracle and to central differences, the optimizer plumbing to hand-written numbers,
the two new exports to the header, and the fixtures of tests/test_gpu_head_train.py to the guard that keeps that test from passing
vacuously."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd import _lib
from tests import _head_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("W,s", [(45, 15), (50, 16)])
def test_reference_forward_equals_oracle(W, s):
    c = R.make_case(W, s, 3, "idx", "mse")
    ref = R.head_loss(c["weights"], c["l"], c["r"], c["targets"], s, "mse", grad=False)
    for p in range(3):
        h = E.head_pair(c["l"][p], c["r"][p], c["weights"], s)
        for k in ("o2", "o3"):
            assert np.max(np.abs(ref[k][p] - h[k])) <= 1e-12 * np.max(np.abs(h[k])), (k, p)
        assert abs(ref["logit"][p] - h["logit"]) <= 1e-12 * max(1.0, abs(h["logit"]))


@pytest.mark.parametrize("W,s,loss", [(45, 15, "sigmoid"), (50, 16, "mse")])
def test_reference_gradients_match_central_differences(W, s, loss):
    """40 seeded coordinates per gradient tensor, h = 1e-6, agreement 1e-6 of the tensor's largest entry: autograd is not the only
    witness of the yardstick."""
    c = R.make_case(W, s, 3, "idx", loss)
    ref = R.head_loss(c["weights"], c["l"], c["r"], c["targets"], s, loss, scale=5.0)
    rng = np.random.default_rng(11)
    h = 1e-6
    for name in R.HEAD_PARAMS:
        g = ref["grads"][name]
        gmax = float(np.abs(g).max())
        coords = rng.choice(g.size, size=min(40, g.size), replace=False)
        for flat in coords:
            vals = []
            for sign in (+1, -1):
                w = {k: np.asarray(v, np.float64) for k, v in c["weights"].items() if k in R.HEAD_PARAMS}
                w[name] = w[name].copy()
                w[name].reshape(-1)[flat] += sign * h
                vals.append(R.head_loss(w, c["l"], c["r"], c["targets"], s, loss, scale=5.0, grad=False)["loss"])
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g.reshape(-1)[flat]) <= 1e-6 * gmax, (name, int(flat), fd, float(g.reshape(-1)[flat]))


def test_negated_differences_flip_the_c_conv1_gradient_only():
    c = R.make_case(45, 15, 3, "idx", "mse")
    w = dict(c["weights"])
    a = R.head_loss(w, c["l"], c["r"], c["targets"], 15, "mse", negate=True)
    w["c_conv1/kernel"] = -w["c_conv1/kernel"]
    b = R.head_loss(w, c["l"], c["r"], c["targets"], 15, "mse")
    for name in R.HEAD_PARAMS:
        sign = -1.0 if name == "c_conv1/kernel" else 1.0
        assert np.allclose(a["grads"][name], sign * b["grads"][name], rtol=1e-12, atol=0), name


def test_lr_schedule_and_adagrad_by_hand():
    from overlapnet_amd.train import adagrad_step, lr_schedule, epoch_batches
    assert lr_schedule(0, 1e-3, 0.99) == pytest.approx(1e-4, rel=1e-15)
    assert lr_schedule(1, 1e-3, 0.99) == pytest.approx(1e-3, rel=1e-15)
    assert lr_schedule(3, 1e-3, 0.5) == pytest.approx(2.5e-4, rel=1e-15)
    p = [torch.tensor([1.0, -2.0], dtype=torch.float64)]
    a = [torch.tensor([0.0, 9.0], dtype=torch.float64)]
    g = [torch.tensor([3.0, 4.0], dtype=torch.float64)]
    adagrad_step(p, a, g, 0.5)
    assert a[0].tolist() == [9.0, 25.0]
    assert p[0].tolist() == [1.0 - 0.5 * 3.0 / (3.0 + 1e-7), -2.0 - 0.5 * 4.0 / (5.0 + 1e-7)]
    adagrad_step(p, a, [torch.tensor([0.0, 0.0], dtype=torch.float64)], 0.5)
    assert a[0].tolist() == [9.0, 25.0]
    b = epoch_batches(10, 4, 2, seed=3)
    assert [len(x) for x in b] == [4, 4, 2] and sorted(np.concatenate(b).tolist()) == list(range(10))
    assert all(np.array_equal(x, y) for x, y in zip(b, epoch_batches(10, 4, 2, seed=3)))
    assert not np.array_equal(np.concatenate(b), np.concatenate(epoch_batches(10, 4, 3, seed=3)))


def test_abi_of_the_gradient_entry_points():
    with open(os.path.join(ROOT, "include", "ovn_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint ovn_head_param_sizes\(ovn_ctx\* ctx, int64_t\* sizes8\);", header)
    assert re.search(r"\bint ovn_delta_head_grad\(ovn_ctx\* ctx,", header)
    m = re.search(r"#define OVN_GRAD_PAIR_BLOCK (\d+)", header)
    assert m and int(m.group(1)) == R.PAIR_BLOCK
    assert re.search(r"#define OVN_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11
    assert "ovn_head_param_sizes" in _lib.SIGNATURES and "ovn_delta_head_grad" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ovn_delta_head_grad"][1]) == 15
    lib = _lib.load()
    assert lib.ovn_abi_version() == 11
    assert lib.ovn_head_param_sizes(None, None) == 1
    assert lib.ovn_delta_head_grad(None, None, None, None, None, 1, None, 0, 1.0, None, None, None, None, None, None) == 1
    assert b"NULL" in lib.ovn_last_error()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_fixture_guard(case):
    """Every fixture of the GPU test, in fp64: gradients that are not tiny, overlaps on the sigmoid's slope and away from their
    targets, about half of the ReLU units active, and no more than 0.1 % of them within the GPU's error bound of zero."""
    c, ref = R.reference(case)
    for name in R.HEAD_PARAMS:
        assert np.abs(ref["grads"][name]).max() > 1e-6, name
    assert np.all(ref["y"] > 0.02) and np.all(ref["y"] < 0.98), ref["y"]
    assert np.all(np.abs(ref["y"] - c["targets"]) > 1e-3)
    for k in ("o2", "o3"):
        assert 0.10 < float((ref[k] > 0).mean()) < 0.90, k
    for k, frac in R.undecided_fraction(c, ref).items():
        assert frac <= 1e-3, (k, frac)


def test_trajectory_fixture_keeps_its_masks_for_six_steps():
    """The trainer test follows the fp64 trajectory while the fp32 restatement keeps the same ReLU masks: at least 6 of the 12 steps
    for the committed seed, and a loss that falls."""
    t = R.trajectory()
    assert t["steps_with_equal_masks"] >= 6
    assert t["losses64"][-1] < t["losses64"][0]


def test_sharded_infer_is_refused():
    import types
    from overlapnet_amd.train import OverlapHeadTrainer
    with pytest.raises(_lib.OvnError, match="sharded"):
        OverlapHeadTrainer(types.SimpleNamespace(_world=2), 1e-3)
