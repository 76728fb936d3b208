"""CPU: guards of the yardstick tests/_leg_grad_ref.py, which tests/test_gpu_leg_train.py holds the leg's backward pass to.

  - without forced masks the restated leg is oracle.overlapnet_oracle.leg_forward;
  - its gradients match central differences in fp64 on a tiny leg;
  - the whole network differentiated end to end equals the chained form the trainer uses (leg forward -> per-pair feature
    gradients -> rows summed per scan for both sides -> leg backward);
  - on the trainer fixture the fp64 loss of the fixed batch after the fixture's Adagrad steps is below its start: the reference
    alone meets the condition the GPU test asserts;
  - the binding and the header agree on the new entry points and on OVN_LEG_GRAD_SCAN_BLOCK."""
import os
import re

import numpy as np
import torch

from oracle import overlapnet_oracle as O
from overlapnet_amd import _lib
from overlapnet_amd import weights as WT
from tests import _head_grad_ref as R
from tests import _leg_grad_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = (19, 61)          # -> s_conv1 8 x 24, s_conv2 3 x 10: two layers with both strides and an uncovered input row / column


def _tiny(seed=0):
    rng = np.random.default_rng(seed)
    layers = WT.leg_layers(4)[:2]
    params = []
    for l in layers:
        params += [rng.normal(0, 0.3, (l.kh, l.kw, l.cin, l.cout)), rng.normal(0, 0.3, l.cout)]
    return layers, params, rng.normal(0, 1, (2,) + TINY + (4,))


def test_header_constant_and_binding():
    src = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    assert int(re.search(r"#define OVN_LEG_GRAD_SCAN_BLOCK (\d+)", src).group(1)) == L.SCAN_BLOCK
    from overlapnet_amd.engine import OvnEngine
    assert OvnEngine.LEG_GRAD_SCAN_BLOCK == L.SCAN_BLOCK
    for name in ("ovn_leg_layer_count", "ovn_leg_param_sizes", "ovn_leg_activation_sizes", "ovn_leg_forward_train", "ovn_leg_backward",
                 "ovn_set_leg_layer_weights", "ovn_debug_conv_grad"):
        assert name in _lib.SIGNATURES, name


def test_argument_errors_without_a_context():
    """NULL contexts and buffers are refused before any HIP call (this machine needs no GPU for it)."""
    lib = _lib.load()
    assert lib.ovn_leg_layer_count(None, None) == 1
    assert lib.ovn_leg_param_sizes(None, None) == 1
    assert lib.ovn_leg_activation_sizes(None, None) == 1
    assert lib.ovn_leg_forward_train(None, None, 1, None, None) == 1
    assert lib.ovn_leg_backward(None, None, None, 1, None, None, 0, None) == 1
    assert lib.ovn_set_leg_layer_weights(None, 0, None, None, None) == 1
    assert lib.ovn_debug_conv_grad(None, 0, None, None, None, 1, 8, 32, None, None, None, None) == 1
    assert b"NULL argument" in lib.ovn_last_error()


def test_restated_leg_is_the_oracle_leg():
    cfg = R.model_cfg(45, 15)
    h, w = R.GEOMS[(45, 15)]
    rng = np.random.default_rng(3)
    x = L.make_images(rng, 2, h, w, 4)
    wts = L.leg_weights(4, cfg)
    names = L.leg_names(4, cfg)
    for dtype, odt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        acts = L.leg_forward([torch.tensor(wts[k], dtype=dtype) for k in names], torch.tensor(x, dtype=dtype), WT.leg_layers(4, cfg))
        assert np.array_equal(acts[-1].numpy(), O.leg_forward(x, wts, cfg, dtype=odt))
    alive = float((acts[-1] > 0).float().mean())
    assert 0.2 < alive < 0.8, alive            # the fixture's last layer is neither dead nor all alive


def test_gradients_match_central_differences():
    layers, params, x = _tiny()
    rng = np.random.default_rng(1)

    def run(ps, masks=None):
        return L.leg_forward([torch.tensor(p, dtype=torch.float64) for p in ps], torch.tensor(x, dtype=torch.float64), layers, masks)
    acts = run(params)
    masks = [(a > 0).numpy() for a in acts]
    d = rng.normal(0, 1, acts[-1].shape)
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in params]
    out = L.leg_forward(tp, torch.tensor(x, dtype=torch.float64), layers, masks)[-1]
    grads = torch.autograd.grad((out * torch.tensor(d)).sum(), tp)
    eps = 1e-6
    for pi, (p, g) in enumerate(zip(params, grads)):
        for _ in range(6):
            idx = tuple(int(rng.integers(0, s)) for s in p.shape)
            hi, lo = [q.copy() for q in params], [q.copy() for q in params]
            hi[pi][idx] += eps
            lo[pi][idx] -= eps
            fd = float(((run(hi, masks)[-1] - run(lo, masks)[-1]) * torch.tensor(d)).sum()) / (2 * eps)
            assert abs(fd - float(g[idx])) <= 1e-6 * max(1.0, abs(fd)), (pi, idx, fd, float(g[idx]))
    # the single-layer form used for ovn_debug_conv_grad, input gradient included
    l0 = layers[0]
    lg = L.layer_grads(params[0], params[1], x, masks[0], rng.normal(0, 1, acts[0].shape), (l0.sh, l0.sw))
    assert lg["din"].shape == x.shape and lg["dkernel"].shape == params[0].shape
    # (19 - 5) % 2 == 0 and (61 - 15) % 2 == 0: covered; one more row / column is not
    x2 = np.concatenate([x, x[:, :1]], axis=1)
    x2 = np.concatenate([x2, x2[:, :, :1]], axis=2)
    out2, _ = L.conv_layer(torch.tensor(x2), torch.tensor(params[0]), torch.tensor(params[1]), (2, 2))
    lg2 = L.layer_grads(params[0], params[1], x2, (out2 > 0).numpy(), rng.normal(0, 1, out2.shape), (2, 2))
    assert np.all(lg2["din"][:, -1] == 0) and np.all(lg2["din"][:, :, -1] == 0) and np.any(lg2["din"][:, -2] != 0)


def test_end_to_end_equals_the_chained_form():
    x = L.trainer_inputs()
    t = L.TRAINER
    e2e = L.network_loss(x["weights"], x["images"], x["left"], x["right"], x["targets"], x["bins"], t["s"], x["cfg"], t["loss"])
    ch = L.chained_grads(x["weights"], x["images"], x["left"], x["right"], x["targets"], x["bins"], t["s"], x["cfg"], t["loss"])
    assert set(ch) == set(e2e["grads"]) and len(ch) == 8 + 2 * 10
    for k, g in e2e["grads"].items():
        scale = float(np.max(np.abs(g)))
        assert scale > 0, k
        assert float(np.max(np.abs(ch[k] - g))) <= 1e-10 * scale, k
    # scan 1 is left in one pair, right in another and both sides of a third: the fixture exercises the shared leg
    assert 1 in x["left"] and 1 in x["right"]
    assert np.any(x["targets"] > 0.7) and np.any(x["targets"] <= 0.7)


def test_trainer_fixture_descends_in_fp64():
    losses = L.trainer_losses64()
    assert len(losses) == L.TRAINER["steps"] + 1
    assert losses[-1] < losses[0], losses
