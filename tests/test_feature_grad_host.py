"""Host side of `ovn_heads_feature_grad` (no GPU): the torch restatement the GPU is measured against (tests/_feature_grad_ref.py) is
pinned to the oracle's literal correlation, to the yaw loss written out with numpy.logaddexp and to central differences; the
fixtures of tests/test_gpu_feature_grad.py are held to the conditions that keep that test from passing vacuously; the export."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import overlapnet_oracle as O
from overlapnet_amd import _lib
from tests import _feature_grad_ref as F
from tests import _head_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["-".join(str(v) for v in c) for c in F.CASES]


@pytest.mark.parametrize("W", [45, 50, 360])
def test_correlation_equals_the_literal_layer(W):
    rng = np.random.default_rng(W)
    l, r = rng.normal(size=(2, W, 128)), rng.normal(size=(2, W, 128))
    z = F.corr_logits(torch.tensor(l), torch.tensor(r)).numpy()
    lit = O.correlation_literal(l[:, None], r[:, None], "none")[:, 0, :, 0]
    terms = np.abs(l).sum() * np.abs(r).max()          # far above any sum of |products| of one logit
    assert np.max(np.abs(z - lit)) <= 1e-13 * terms
    assert np.max(np.abs(z - lit)) <= 1e-12 * np.max(np.abs(lit))


def test_yaw_loss_equals_the_formula_with_logaddexp():
    W = 45
    rng = np.random.default_rng(5)
    z = rng.normal(0, 6, size=(4, W))
    z[0, :4] = [0.0, -40.0, 40.0, 1e-9]
    bins, targets = [3, W - 1, -1, 0], np.array([0.9, 0.71, 0.9, 0.7], np.float32)
    q = F.yaw_targets(bins, targets, W)
    assert q.sum(axis=1).tolist() == [1.0, 1.0, 0.0, 0.0] and q[0, 3] == 1 and q[1, W - 1] == 1
    got = F.yaw_loss_terms(torch.tensor(z), torch.tensor(q), W).numpy()
    # -log sigmoid(z) = logaddexp(0, -z), -log(1 - sigmoid(z)) = logaddexp(0, z)
    want = W * q * np.logaddexp(0.0, -z) + (1.0 - q) * np.logaddexp(0.0, z)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


@pytest.mark.parametrize("W,s,n,loss", [(45, 15, 5, "sigmoid"), (50, 16, 3, "mse")])
def test_gradients_match_central_differences(W, s, n, loss):
    """24 seeded elements of l and of r with l != r along the element's whole row of differences (|.| is smooth there), per loss;
    h = 1e-7 (the scaled volumes are of the order 0.05), agreement 1e-5 of the tensor's largest entry."""
    c, ref = F.reference((W, s, n, "idx", loss))
    rng = np.random.default_rng(3)
    h = 1e-7
    R_ = (W // s) * s
    for which in ("l", "r"):
        x, other = c[which].astype(np.float64), c["r" if which == "l" else "l"].astype(np.float64)
        done = 0
        while done < 24:
            p, i, ch = int(rng.integers(0, n)), int(rng.integers(0, W)), int(rng.integers(0, 128))
            if np.any(np.abs(x[p, i, ch] - other[p, :R_, ch]) <= 4 * h):
                continue
            vals = {}
            for sign in (+1, -1):
                y = x.copy()
                y[p, i, ch] += sign * h
                args = (y, other) if which == "l" else (other, y)
                f = F.feature_loss(c["weights"], args[0], args[1], c["targets"], c["bins"], s, loss, grad=False)
                vals[sign] = (f["loss_overlap"], f["loss_yaw"])
            for k, part in enumerate(("overlap", "yaw")):
                g = ref["d" + which][part]
                fd = (vals[1][k] - vals[-1][k]) / (2 * h)
                assert abs(fd - g[p, i, ch]) <= 1e-5 * np.abs(g).max(), (which, part, p, i, ch, fd, float(g[p, i, ch]))
            done += 1


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_fixture_conditions(case):
    W, s, n, form, loss = case
    c, ref = F.reference(case)
    assert float((np.abs(ref["z"]) <= 8).mean()) >= 0.5
    if n >= 2:
        assert np.any(c["targets"] > F.THRESHOLD) and np.any(c["targets"] <= F.THRESHOLD)
    if form == "idx" and n > 1:
        assert len(set(c["lidx"])) < n or len(set(c["ridx"])) < n
    same = 0
    for p in range(n):                                  # (i, j, c) triples with l == r, a pair at a time
        same += int((c["l"][p][:, None, :] == c["r"][p][None, :, :]).sum())
    assert same >= 0.05 * n * W * W * 128
    for k, frac in R.undecided_fraction(c, ref).items():
        assert frac <= 1e-3, (k, frac)
    for part in ("overlap", "yaw"):                     # gradients that are not tiny
        assert np.abs(ref["dl"][part]).max() > 1e-4 and np.abs(ref["dr"][part]).max() > 1e-4, part


def test_fixtures_cover_the_edge_bins_and_the_self_pair():
    bins = {(int(b), c[0]) for c in F.CASES for b in F.make_case(c)["bins"]}
    for W in {c[0] for c in F.CASES if c[0] != 360}:
        assert {(0, W), (W - 1, W), (W // 2, W)} <= bins, W
    c, ref = F.reference(F.SELF_PAIR_CASE)
    assert c["lidx"][1] == c["ridx"][1] and np.array_equal(c["l"][1], c["r"][1])
    assert not np.any(ref["dl"]["overlap"][1]) and not np.any(ref["dr"]["overlap"][1])
    assert np.any(ref["dl"]["yaw"][1])


def test_the_entry_point_is_exported_and_bound():
    with open(os.path.join(ROOT, "include", "ovn_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint ovn_heads_feature_grad\(ovn_ctx\* ctx,", header)
    assert re.search(r"#define OVN_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11
    assert len(_lib.SIGNATURES["ovn_heads_feature_grad"][1]) == 19
    lib = _lib.load()
    assert lib.ovn_abi_version() == 11
    args = [None] * 5 + [1, None, None, 0, 5.0, 1.0, 0.7] + [None] * 7
    assert lib.ovn_heads_feature_grad(*args) == 1
    assert b"NULL" in lib.ovn_last_error()
    from overlapnet_amd import train
    from overlapnet_amd.engine import OvnEngine
    assert callable(train.heads_loss) and callable(OvnEngine.heads_feature_grad)


def test_sum_rows_by_entry_adds_in_pair_order():
    from overlapnet_amd.train import sum_rows_by_entry
    rows = torch.tensor([[1e8], [1.0], [-1e8], [2.0], [3.0]], dtype=torch.float32)
    out = sum_rows_by_entry(rows, [2, 0, 2, 2, 0], 4)
    want = [np.float32(1.0) + np.float32(3.0), 0.0, (np.float32(1e8) + np.float32(-1e8)) + np.float32(2.0), 0.0]
    assert out.reshape(-1).tolist() == [float(v) for v in want]
    assert torch.equal(out, sum_rows_by_entry(rows, torch.tensor([2, 0, 2, 2, 0]), 4))
