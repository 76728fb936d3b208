"""GPU (MI355X): the leg's backward pass (`ovn_leg_backward`, `ovn_debug_conv_grad`, csrc/leg_backward.hip), the training forward,
`ovn_set_leg_layer_weights` and `train.OverlapNetTrainer`, against the fp64 restatement of tests/_leg_grad_ref.py.

Tolerance (the project's own, DESIGN.md sections 19 - 21): the GPU's ReLU masks (stored activation > 0) are forced into the
reference, and every gradient tensor stays within 4 T of fp64, T = max |g32 - g64| of the same restatement in float32 on the CPU
with the same masks.  With OVN_LEG_TRAIN_PARITY_JSON set, the measured ratios max |g_gpu - g64| / T are written to that file.

  1. each layer alone, all 11 layer shapes of the `additional_unsymmetric_layer3a` leg, three inputs per layer:
       'few'    1 x 5 output pixels, nb = 1: fewer than one MFMA tile of pixels;
       'odd'    2 x 37 output pixels from an input with one row (and, for a column stride of 2, one column) more than the windows
                cover -- (h - kh) % sh == 1 where sh == 2 -- whose data gradient must be exactly zero there; 74 pixels are no multiple
                of 16; nb = OVN_LEG_GRAD_SCAN_BLOCK + 1: two scan blocks, the first of 296 pixels = two reduction pieces of 256;
       'long'   2 x 150 output pixels in one scan: more than one reduction piece inside a scan;
     plus layer 0 at 1 and 5 input channels (K = 75 and 375: no multiple of 4 or 16).  dX, dW, db within 4 T, the same bits twice.
  2. the training forward: every stored activation within oracle.error_bounds.leg_layer_bound(..., 'f32') of the fp64 layer applied
     to the GPU's own previous activation; the last block is BITWISE `engine.leg` under leg precision 'f32' (both run
     ovn_conv_forward of conv_f32.hip layer by layer, and a pixel's sum does not depend on the batch).
  3. the whole leg at (32, 247) -> W = 45 and (32, 311) -> W = 77 (n = 1, 3, block + 1) and (64, 900) with 3a (n = 2): all gradients
     within 4 T; the same bits twice and for slice_scans = one block.
  4. `set_leg_weights`: `engine.leg` in both precisions equals a fresh engine's loaded with the same weights.
  5. the trainer: gradients of all 8 + 2 x layers tensors within 4 T of the fp64 whole network on a batch with a scan shared between a left and
     a right slot; one step = `adagrad_step` on those gradients; the fixed batch's loss falls; the saved file reproduces
     `infer_one` bitwise; the cache is empty and the look-ahead closed afterwards; train_legs=False leaves the legs untouched.
  6. argument errors of every new entry point, before any launch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd import _lib
from overlapnet_amd import weights as WT
from tests import _head_grad_ref as R
from tests import _leg_geometry_ref as G
from tests import _leg_grad_ref as L

pytestmark = pytest.mark.gpu

_RATIOS = {}
SB = L.SCAN_BLOCK
CFG3A = {"additional_unsymmetric_layer3a": True}


@pytest.fixture(scope="module")
def parity_file():
    yield
    path = os.environ.get("OVN_LEG_TRAIN_PARITY_JSON")
    if path and _RATIOS:
        with open(path, "w") as f:
            json.dump({"what": "max |g_gpu - g64| / max |g32_cpu - g64| per tensor (pass: <= 4)", "worst": max(_RATIOS.values()),
                       "ratios": _RATIOS}, f, indent=1, sort_keys=True)


def _within_4T(tag, name, gpu, g32, g64):
    g64 = np.asarray(g64, np.float64)
    T = float(np.max(np.abs(np.asarray(g32, np.float64) - g64)))
    err = float(np.max(np.abs(np.asarray(gpu, np.float64).reshape(g64.shape) - g64)))
    ratio = err / T if T > 0 else (0.0 if err == 0 else float("inf"))
    _RATIOS["%s %s" % (tag, name)] = ratio
    print("%-28s %-18s T %.3e  gpu err %.3e  ratio %.3f" % (tag, name, T, err, ratio))
    assert np.all(np.isfinite(np.asarray(gpu))), (tag, name)
    assert err <= 4 * T, (tag, name, err, T)


def _engine(h, w, c, weights, cfg):
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(h, w, c)
    try:
        e.load_weights(weights, cfg)
    except Exception:
        e.close()
        raise
    return e


@pytest.fixture(scope="module")
def eng3a():
    w = L.leg_weights(4, CFG3A, seed=0, feat_w=360)
    e = _engine(64, 900, 4, w, CFG3A)
    yield e, w
    e.close()


# ---- 1. each layer alone ---------------------------------------------------------------------------------------------------------

_layer_inputs = G.layer_inputs      # name -> (nb, h, w) for one layer (see the module docstring); any stride: stride - 1 uncovered rows / columns


def _check_layer(eng, weights, li, l, which, tag):
    """Layer `l` (index li of `eng`: an OvnEngine, or a `_leg_geometry_ref.LayerEngine` holding the one layer) on input `which`."""
    nb, h, w = _layer_inputs(l)[which]
    oh, ow = (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1
    assert (oh, ow) == {"few": (1, 5), "odd": (2, 37), "long": (2, 150)}[which]
    x, dout = G.backward_data(li, l, which)
    xt, dt = torch.from_numpy(x).to(eng.device), torch.from_numpy(dout).to(eng.device)
    eng.set_leg_precision("f32")
    out = eng.debug_conv(li, xt)
    mask = (out > 0).cpu().numpy()
    assert 0.2 < mask.mean() < 0.8
    g = eng.debug_conv_grad(li, xt, out, dt)
    g2 = eng.debug_conv_grad(li, xt, out, dt)
    for k in ("din", "dkernel", "dbias"):
        assert torch.equal(g[k], g2[k]), (tag, k, "twice")
    only = eng.debug_conv_grad(li, xt, out, dt, want=("dkernel",))
    assert set(only) == {"dkernel"} and torch.equal(only["dkernel"], g["dkernel"])
    kern, bias = weights[l.name + "/kernel"], weights[l.name + "/bias"]
    r64 = L.layer_grads(kern, bias, x, mask, dout, (l.sh, l.sw), torch.float64)
    r32 = L.layer_grads(kern, bias, x, mask, dout, (l.sh, l.sw), torch.float32)
    for k in ("din", "dkernel", "dbias"):
        _within_4T(tag, k, g[k].cpu().numpy(), r32[k], r64[k])
    din = g["din"].cpu().numpy()
    ch, cw = (oh - 1) * l.sh + l.kh, (ow - 1) * l.sw + l.kw          # rows / columns some window covers
    if which == "odd":
        assert ch == h - (l.sh - 1) and cw == w - (l.sw - 1)
    assert np.all(din[:, ch:] == 0) and np.all(din[:, :, cw:] == 0), tag
    assert np.any(din[:, ch - 1] != 0) and np.any(din[:, :, cw - 1] != 0), tag
    if l.sh <= l.kh:                                                  # no gaps between the windows: every covered row gets a gradient
        assert np.all(np.any(din[:, :ch] != 0, axis=(0, 2, 3))), tag
    if l.sw <= l.kw:
        assert np.all(np.any(din[:, :, :cw] != 0, axis=(0, 1, 3))), tag


LAYERS3A = WT.leg_layers(4, CFG3A)


@pytest.mark.parametrize("which", ("few", "odd", "long"))
@pytest.mark.parametrize("li", range(len(LAYERS3A)), ids=[l.name for l in LAYERS3A])
def test_each_layer_alone(li, which, eng3a, parity_file):
    eng, w = eng3a
    assert len(LAYERS3A) == 11
    _check_layer(eng, w, li, LAYERS3A[li], which, "%s %s" % (LAYERS3A[li].name, which))


@pytest.mark.parametrize("in_c", (1, 5))
def test_first_layer_at_other_channel_counts(in_c, parity_file):
    cfg = R.model_cfg(45, 15)
    w = L.leg_weights(in_c, cfg, seed=in_c, feat_w=45)
    eng = _engine(32, 247, in_c, w, cfg)
    try:
        l = WT.leg_layers(in_c, cfg)[0]
        assert (l.kh * l.kw * l.cin) % 4 != 0
        for which in ("few", "odd", "long"):
            _check_layer(eng, w, 0, l, which, "s_conv1 C=%d %s" % (in_c, which))
    finally:
        eng.close()


# ---- 2. / 3. the training forward and the whole leg -------------------------------------------------------------------------------

LEG_CASES = [(45, n) for n in (1, 3, SB + 1)] + [(77, n) for n in (1, 3, SB + 1)] + [(360, 2)]


def _whole_leg(cfg, h, wi, W, n, tag, seed=None):
    """The training forward and the whole leg's backward pass for model section `cfg` on n scans of h x wi (feature width W)."""
    layers = WT.leg_layers(4, cfg)
    rng = np.random.default_rng([W, n, 5])
    weights = L.leg_weights(4, cfg, seed=W if seed is None else seed, feat_w=W)
    images = L.make_images(rng, n, h, wi, 4)
    eng = _engine(h, wi, 4, weights, cfg)
    try:
        assert eng.feat_w == W
        shapes = eng.leg_param_shapes()
        assert shapes == [tuple(weights[k].shape) for k in L.leg_names(4, cfg)]
        x = torch.from_numpy(images).to(eng.device)
        eng.set_leg_precision("f16x3")                       # the training forward is fp32 whatever the mode says
        acts = eng.leg_forward_train(x)
        eng.set_leg_precision("f32")
        assert torch.equal(acts[-1].view(n, W, 128), eng.leg(x))
        host = [a.cpu().numpy() for a in acts]
        # 2. every stored activation against the fp64 layer on the GPU's own previous activation
        if n <= 3:
            prev = images
            for l, a in zip(layers, host):
                want, b = E.leg_layer_bound(prev, weights[l.name + "/kernel"], weights[l.name + "/bias"], (l.sh, l.sw), modes=("f32",))
                assert a.shape == want.shape
                worst = E.ratio(a, want, b["f32"])
                print("forward %-9s worst error / bound %.3f" % (l.name, worst))
                assert worst <= 1.0, l.name
                prev = a
        # 3. the gradients
        alive = host[-1] > 0
        assert 0.2 < alive.mean() < 0.8
        dfeat = L.random_dfeat(rng, host[-1].reshape(n, W, 128))
        d = torch.from_numpy(dfeat).to(eng.device)
        g = eng.leg_backward(x, acts, d)
        assert torch.equal(g["flat"], eng.leg_backward(x, acts, d)["flat"]), "twice"
        assert torch.equal(g["flat"], eng.leg_backward(x, acts, d, slice_scans=SB)["flat"]), "slices of one block"
        if n > SB:
            assert torch.equal(g["flat"], eng.leg_backward(x, acts, d, slice_scans=1)["flat"]), "slice_scans below a block"
        masks = [a > 0 for a in host]
        g64, _ = L.leg_grads(weights, images, dfeat, cfg, torch.float64, masks)
        g32, _ = L.leg_grads(weights, images, dfeat, cfg, torch.float32, masks)
        for name in L.leg_names(4, cfg):
            assert tuple(g[name].shape) == g64[name].shape
            _within_4T(tag, name, g[name].cpu().numpy(), g32[name], g64[name])
    finally:
        eng.close()


@pytest.mark.parametrize("W,n", LEG_CASES, ids=["W%d-n%d" % c for c in LEG_CASES])
def test_whole_leg(W, n, parity_file):
    cfg = R.model_cfg(W, 15)
    h, wi = R.GEOMS[(W, 15)]
    assert len(WT.leg_layers(4, cfg)) == (11 if W == 360 else 10)
    _whole_leg(cfg, h, wi, W, n, "leg W%d n%d" % (W, n))


# ---- 4. set_leg_weights -------------------------------------------------------------------------------------------------------------

def test_set_leg_weights_equals_a_fresh_engine(eng3a):
    eng, w0 = eng3a
    w1 = dict(w0)
    w1.update({k: v for k, v in L.leg_weights(4, CFG3A, seed=9, feat_w=360).items() if k.startswith("s_conv")})
    rng = np.random.default_rng(11)
    x = torch.from_numpy(L.make_images(rng, 2, 64, 900, 4)).to(eng.device)
    fresh = _engine(64, 900, 4, w1, CFG3A)
    try:
        eng.set_leg_precision("f32")
        before = eng.leg(x)
        eng.set_leg_weights({k: torch.from_numpy(w1[k]).to(eng.device) for k in L.leg_names(4, CFG3A)})
        for mode in ("f16x3", "f32"):
            eng.set_leg_precision(mode)
            fresh.set_leg_precision(mode)
            assert torch.equal(eng.leg(x), fresh.leg(x)), mode
        assert not torch.equal(before, eng.leg(x))
        assert torch.equal(eng.leg_forward_train(x)[-1].view(2, 360, 128), fresh.leg(x))
        with pytest.raises(_lib.OvnError):                    # a layer needs both of its tensors
            eng.set_leg_weights({"s_conv2/kernel": torch.from_numpy(w1["s_conv2/kernel"]).to(eng.device)})
    finally:
        fresh.close()
        eng.set_leg_weights({k: torch.from_numpy(w0[k]).to(eng.device) for k in L.leg_names(4, CFG3A)})   # the module's engine
        eng.set_leg_precision("f32")


# ---- 5. the trainer ------------------------------------------------------------------------------------------------------------------

def _infer_cfg(root, weights_file="", **model_extra):
    t = L.TRAINER
    return {"model": dict(R.model_cfg(t["W"], t["s"]), **model_extra), "infer_seqs": "07", "data_root_folder": str(root),
            "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
            "use_intensity": False, "batch_size": 8, "pretrained_weightsfilename": weights_file, "precision": "f32",
            "stream_ahead": False}


@pytest.fixture()
def scans(tmp_path):
    """The trainer fixture's images as the cue files `Infer` reads; -> (root, inputs, names)."""
    x = L.trainer_inputs()
    seq = tmp_path / "data" / "07"
    for sub in ("depth", "normal"):
        os.makedirs(seq / sub)
    names = ["%06d" % i for i in range(x["images"].shape[0])]
    for i, name in enumerate(names):
        np.save(seq / "depth" / (name + ".npy"), np.ascontiguousarray(x["images"][i, :, :, 0]))
        np.save(seq / "normal" / (name + ".npy"), np.ascontiguousarray(x["images"][i, :, :, 1:4]))
    return tmp_path / "data", x, names


def _batch(x, names):
    return [names[i] for i in x["left"]], [names[i] for i in x["right"]], x["targets"], x["bins"]


def test_trainer_gradients_and_one_step(scans, parity_file):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapNetTrainer, adagrad_step, lr_schedule
    root, x, names = scans
    t = L.TRAINER
    inf = Infer(_infer_cfg(root), weights=x["weights"])
    try:
        tr = OverlapNetTrainer(inf, t["lr"], t["alpha"], t["loss"])
        assert len(tr.names) == 8 + 2 * 10 and len(tr.params) == len(tr.names)       # this fixture's leg has no s_conv3a: 28 of the 30
        ln, rn, ov, yb = _batch(x, names)
        g = tr.gradients(ln, rn, ov, yb)
        # the GPU's masks: the leg's stored activations and the head's o2 / o3 on the same pairs
        xd = inf._inputs_device(names)
        assert np.array_equal(xd.cpu().numpy(), x["images"])
        acts = inf.engine.leg_forward_train(xd)
        feats = acts[-1].view(len(names), t["W"], 128)
        head = inf.engine.delta_head_grad(feats, feats, ov, lidx=x["left"], ridx=x["right"], loss=t["loss"], scale=5.0,
                                          want_activations=True)
        leg_masks = [(a > 0).cpu().numpy() for a in acts]
        head_masks = [(head["o2"] > 0).cpu().numpy(), (head["o3"] > 0).cpu().numpy()]
        refs = {dt: L.network_loss(x["weights"], x["images"], x["left"], x["right"], ov, yb, t["s"], x["cfg"], t["loss"], dtype=dt,
                                   leg_masks=leg_masks, head_masks=head_masks) for dt in (torch.float64, torch.float32)}
        for name in tr.names:
            _within_4T("trainer", name, g[name].cpu().numpy(), refs[torch.float32]["grads"][name], refs[torch.float64]["grads"][name])
        r64 = refs[torch.float64]
        assert abs(float(g["loss_overlap"]) - r64["loss_overlap"]) <= 1e-3 * abs(r64["loss_overlap"]) + 1e-6
        assert abs(float(g["loss_yaw"]) - r64["loss_yaw"]) <= 1e-3 * abs(r64["loss_yaw"]) + 1e-6
        # one step = adagrad_step on exactly those gradients
        want = [p.clone() for p in tr.params]
        adagrad_step(want, [torch.zeros_like(p) for p in want], [g[n].reshape(p.shape) for n, p in zip(tr.names, want)],
                     float(lr_schedule(0, t["lr"], t["alpha"])))
        before = [p.clone() for p in tr.params]
        inf.feature_volumes = [np.zeros((1, t["W"], 128), np.float32)]
        loss0 = tr.step(ln, rn, ov, yb)
        assert abs(loss0 - float(g["loss_overlap"] + g["loss_yaw"])) <= 1e-6 * abs(loss0)
        for name, p, w_, b in zip(tr.names, tr.params, want, before):
            assert torch.equal(p, w_), name
            assert not torch.equal(p, b), name
        assert len(inf.feature_volumes) == 0 and inf._qa is None
        for name, p in zip(tr.names, tr.params):
            assert np.array_equal(inf._weights[name].reshape(-1), p.cpu().numpy().reshape(-1)), name
    finally:
        inf.close()


def test_trainer_descends_saves_and_reloads(scans):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapNetTrainer
    root, x, names = scans
    t = L.TRAINER
    path = str(root / "trained.npz")
    inf = Infer(_infer_cfg(root), weights=x["weights"])
    try:
        tr = OverlapNetTrainer(inf, t["lr"], t["alpha"], t["loss"])
        ln, rn, ov, yb = _batch(x, names)
        losses = [tr.step(ln, rn, ov, yb) for _ in range(t["steps"])]
        g = tr.gradients(ln, rn, ov, yb)
        losses.append(float(g["loss_overlap"] + g["loss_yaw"]))
        ref = L.trainer_losses64()
        for k, (a, b) in enumerate(zip(losses, ref)):
            print("step %d  gpu %.6f  fp64 %.6f" % (k, a, b))
        assert losses[-1] < losses[0]
        tr.save(path)
        mine = inf.infer_one("000000.bin", "000001.bin")
        # fit: one epoch of two mini-batches; the cache is emptied and the look-ahead closed
        inf.feature_volumes = [np.zeros((1, t["W"], 128), np.float32)] * 2
        out = tr.fit(ln, rn, ov, yb, epochs=1, batch_size=4)
        assert len(out) == 2 and tr.epoch == 1
        assert len(inf.feature_volumes) == 0 and inf._qa is None
    finally:
        inf.close()
    fresh = Infer(_infer_cfg(root, weights_file=path))
    try:
        theirs = fresh.infer_one("000000.bin", "000001.bin")
    finally:
        fresh.close()
    assert np.array_equal(np.asarray(mine[0]).view(np.uint32), np.asarray(theirs[0]).view(np.uint32))
    assert np.array_equal(mine[1], theirs[1])


def test_trainer_with_frozen_legs_and_negated_differences(scans):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.train import OverlapNetTrainer
    root, x, names = scans
    t = L.TRAINER
    inf = Infer(_infer_cfg(root, deltaLayer_negateDiffs=True), weights=x["weights"])
    try:
        tr = OverlapNetTrainer(inf, t["lr"], t["alpha"], t["loss"], train_legs=False)
        ln, rn, ov, yb = _batch(x, names)
        xd = inf._inputs_device(names)
        feats_before = inf.engine.leg(xd).clone()
        g = tr.gradients(ln, rn, ov, yb)
        assert set(g) == set(R.HEAD_PARAMS) | {"loss_overlap", "loss_yaw", "overlap"}
        tr.step(ln, rn, ov, yb)
        after = tr.weights()
        for k in L.leg_names(4, x["cfg"]):
            assert np.array_equal(after[k], x["weights"][k]), k
        assert torch.equal(inf.engine.leg(xd), feats_before)
        assert not np.array_equal(after["c_conv1/kernel"], x["weights"]["c_conv1/kernel"])
        # the file's kernel moves against the file's gradient (the sign of the registered, negated kernel is undone on both)
        step = after["c_conv1/kernel"] - x["weights"]["c_conv1/kernel"]
        gf = g["c_conv1/kernel"].cpu().numpy()
        moved = step != 0
        assert moved.mean() > 0.5
        assert np.all(np.sign(step[moved]) == -np.sign(gf[moved]))
    finally:
        inf.close()


def test_trainer_refuses_a_sharded_infer():
    from overlapnet_amd.train import OverlapNetTrainer

    class Sharded(object):
        _world = 2
    with pytest.raises(_lib.OvnError):
        OverlapNetTrainer(Sharded(), 1e-3)


# ---- 6. argument errors ----------------------------------------------------------------------------------------------------------------

def test_argument_errors(eng3a):
    from overlapnet_amd.engine import OvnEngine, _ptr
    eng, w = eng3a
    lib, h = eng.lib, eng._h
    x = torch.zeros((1, 64, 900, 4), dtype=torch.float32, device=eng.device)
    acts = eng.leg_forward_train(x)
    d = torch.zeros((1, 360, 128), dtype=torch.float32, device=eng.device)
    grad = torch.zeros(sum(int(np.prod(s)) for s in eng.leg_param_shapes()), dtype=torch.float32, device=eng.device)
    ws = eng.workspace_bytes()
    px, pa, pd, pg = _ptr(x), C.c_void_p(acts[0].data_ptr()), _ptr(d), _ptr(grad)
    assert lib.ovn_leg_forward_train(h, None, 1, pa, None) == 1
    assert lib.ovn_leg_forward_train(h, px, 1, None, None) == 1
    assert lib.ovn_leg_forward_train(h, px, 0, pa, None) == 1
    assert lib.ovn_leg_backward(h, None, pa, 1, pd, pg, 0, None) == 1
    assert lib.ovn_leg_backward(h, px, None, 1, pd, pg, 0, None) == 1
    assert lib.ovn_leg_backward(h, px, pa, 1, None, pg, 0, None) == 1
    assert lib.ovn_leg_backward(h, px, pa, 1, pd, None, 0, None) == 1
    assert lib.ovn_leg_backward(h, px, pa, 0, pd, pg, 0, None) == 1
    assert lib.ovn_leg_backward(h, px, pa, -3, pd, pg, 0, None) == 1
    assert lib.ovn_leg_backward(h, px, pa, 1, pd, pg, -1, None) == 1 and b"slice_scans" in lib.ovn_last_error()
    k = torch.from_numpy(w["s_conv1/kernel"]).to(eng.device)
    b = torch.from_numpy(w["s_conv1/bias"]).to(eng.device)
    assert lib.ovn_set_leg_layer_weights(h, 0, None, _ptr(b), None) == 1
    assert lib.ovn_set_leg_layer_weights(h, 0, _ptr(k), None, None) == 1
    assert lib.ovn_set_leg_layer_weights(h, -1, _ptr(k), _ptr(b), None) == 1
    assert lib.ovn_set_leg_layer_weights(h, 11, _ptr(k), _ptr(b), None) == 1
    assert lib.ovn_add_leg_layer(h, b"s_conv11", _ptr(k), _ptr(b), 5, 15, 4, 16, 2, 2, None) == 3      # still refused after finalize
    xi = torch.zeros((1, 5, 19, 4), dtype=torch.float32, device=eng.device)
    yo = torch.zeros((1, 1, 3, 16), dtype=torch.float32, device=eng.device)
    for layer in (-1, 11):
        assert lib.ovn_debug_conv_grad(h, layer, _ptr(xi), _ptr(yo), _ptr(yo), 1, 5, 19, None, None, None, None) == 1
    assert lib.ovn_debug_conv_grad(h, 0, None, _ptr(yo), _ptr(yo), 1, 5, 19, None, None, None, None) == 1
    assert lib.ovn_debug_conv_grad(h, 0, _ptr(xi), None, _ptr(yo), 1, 5, 19, None, None, None, None) == 1
    assert lib.ovn_debug_conv_grad(h, 0, _ptr(xi), _ptr(yo), None, 1, 5, 19, None, None, None, None) == 1
    assert lib.ovn_debug_conv_grad(h, 0, _ptr(xi), _ptr(yo), _ptr(yo), 0, 5, 19, None, None, None, None) == 1
    assert lib.ovn_debug_conv_grad(h, 0, _ptr(xi), _ptr(yo), _ptr(yo), 1, 4, 19, None, None, None, None) == 1   # smaller than the kernel
    n = C.c_int(0)
    assert lib.ovn_leg_layer_count(h, None) == 1 and lib.ovn_leg_layer_count(h, C.byref(n)) == 0 and n.value == 11
    assert lib.ovn_leg_param_sizes(h, None) == 1 and lib.ovn_leg_activation_sizes(h, None) == 1
    assert eng.workspace_bytes() == ws                         # nothing was reserved, nothing ran
    # a context that was never finalized
    bare = OvnEngine(32, 247, 4)
    try:
        sizes = (C.c_int64 * 4)()
        assert lib.ovn_leg_activation_sizes(bare._h, sizes) == 3
        assert lib.ovn_leg_forward_train(bare._h, px, 1, pa, None) == 3
        assert lib.ovn_leg_backward(bare._h, px, pa, 1, pd, pg, 0, None) == 3
        assert lib.ovn_set_leg_layer_weights(bare._h, 0, _ptr(k), _ptr(b), None) == 3
        assert lib.ovn_leg_layer_count(bare._h, C.byref(n)) == 0 and n.value == 0
        with pytest.raises(_lib.OvnError):
            bare.leg_forward_train(x)
    finally:
        bare.close()
    # the Python wrappers refuse what does not fit before they call
    with pytest.raises(_lib.OvnError):
        eng.leg_backward(x, acts[:-1], d)
    with pytest.raises(_lib.OvnError):
        eng.leg_backward(x, acts, d[:, :100])
    with pytest.raises(ValueError):
        eng.leg_backward(x, acts, d, slice_scans=-1)
    with pytest.raises(IndexError):
        eng.debug_conv_grad(11, xi, yo, yo)
