"""CPU: guards of tests/_leg_geometry_ref.py, the table tests/test_gpu_leg_geometry.py runs on the GPU.

  - the shape table holds: every SMALL input gives 1 x 45 and one column less does not, 16 x 900 with [1, 2] gives 1 x 371;
  - the mirrored dispatch reaches every branch the cases are there for (and the shipped 64 x 900 leg reaches none of them);
  - the fp64 ReLU-alive fraction of every case lies in 0.2 - 0.8 (what `_check_layer` / `_whole_leg` of
    tests/test_gpu_leg_train.py assert on the GPU's masks), and the float32 CPU restatement stays inside the forward bound:
    the reference alone meets both, with the seeds of the table;
  - the fp64 restatement's gradients of a strided synthetic layer match central differences, uncovered rows and columns included;
  - the entry points used refuse a NULL context before any HIP call, and the documents state the 128-position rule."""
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd import _lib
from overlapnet_amd import weights as WT
from tests import _leg_geometry_ref as G
from tests import _leg_grad_ref as L
from tools import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_table():
    assert len(G.SMALL) == 6 and {s for s, _ in G.SMALL} == {(1, 1), (1, 2), (2, 1)}
    for (strides, a3), (h, w) in G.SMALL.items():
        cfg = G.small_cfg(strides, a3)
        layers = WT.leg_layers(4, cfg)
        assert len(layers) == (11 if a3 else 10) and (layers[0].sh, layers[0].sw) == strides
        assert WT.leg_output_shape(h, w, layers) == (1, 45, 128), (strides, a3)
        assert WT.feature_width(h, w, 4, cfg, 45) == 45
        assert h in (16, 32, 64)                                     # beam counts of real sensors
        assert WT.leg_output_shape(h, w - 1, layers) == (1, 44, 128)      # the narrowest such input
    strides, a3, (h, w), fw = G.DOCUMENTED
    assert WT.leg_output_shape(h, w, WT.leg_layers(4, G.cfg_of(strides, a3, (h, w), fw))) == (1, fw, 128)
    assert (strides, a3, (h, w), fw) == ((1, 2), False, (16, 900), 371)
    for case in G.BACKWARD:
        assert case in G.SMALL


def test_dispatch_mirror_reaches_every_branch():
    by = {l.name: l for l in G.SYNTH}
    fwd = {l.name: G.forward_f16x3(l, 3, *G.forward_shape(l)[2:]) for l in G.SYNTH}
    bwd = {l.name: {w: G.backward(l, *G.layer_inputs(l)[w]) for w in ("few", "odd", "long")} for l in G.SYNTH}
    for l in G.SYNTH:
        oh, ow, h, w = G.forward_shape(l)
        assert G.out_shape(l, h, w) == (oh, ow) and oh * ow == 136 and 136 >= G.MIN_POSITIONS and 136 % 16 != 0
        assert ((h - l.kh) % l.sh, (w - l.kw) % l.sw) == (l.sh - 1, l.sw - 1)            # the most uncovered rows / columns
        assert l.cout % 16 == 0 and l.cin % 4 == 0
        # every synthetic layer takes the generic f16x3 kernel with the 16-byte gather, also where the 16-tap fragments exist
        assert fwd[l.name]["kernel"] == "conv_mfma_f16x3_kernel" and fwd[l.name]["gather"] == "vec4", l.name
        for which, (nb, hh, ww) in G.layer_inputs(l).items():
            assert G.out_shape(l, hh, ww) == {"few": (1, 5), "odd": (2, 37), "long": (2, 150)}[which]
        assert bwd[l.name]["odd"]["blocks"] == 2 and bwd[l.name]["odd"]["pieces"] == 2 and bwd[l.name]["long"]["pieces"] > 1
    # 1. the MFMA data gradient with a column stride, and with a row stride that is neither 1 nor 2
    mfma = [l for l in G.SYNTH if bwd[l.name]["few"]["dgrad"][0] == "mfma"]
    assert {l.sw for l in mfma} >= {1, 2, 3} and {l.sh for l in mfma} >= {1, 2, 3}
    assert by["g3x5_16_32_s22"] in mfma and by["g4x3_16_32_s32"] in mfma
    assert bwd["g3x3_8_16_s31"]["few"]["dgrad"] == ("plain",) and bwd["g2x2_12_16_s11"]["few"]["dgrad"] == ("plain",)
    # 2. the gather's walk: one select per chunk, and the while wrap for KW Cin < 32
    assert {fwd[n]["wrap"] for n in fwd} == {"select", "while"}
    assert [l.kw * l.cin for l in G.SYNTH if fwd[l.name]["wrap"] == "while"] == [24, 24, 16]
    assert by["g1x1_64_64_s11"].kh * by["g1x1_64_64_s11"].kw == 1 and by["g2x2_12_16_s11"].cin % 8 == 4
    # the default: launch branches (both forward precisions share the switch), and the 128-column tile with two column blocks
    assert fwd["g2x4_32_48_s13"]["tile"] == (2, 1, 4, 1, 3, "default-16")
    assert fwd["g1x9_128_256_s11"]["tile"] == (2, 4, 2, 2, 2, "default-128")
    assert G.generic_tile(by["g1x9_128_256_s11"], 3 * 136, f16x3=False) == (2, 4, 2, 2, 2, "default-128")
    assert {fwd[n]["tile"][5] for n in fwd} == {"case", "default-16", "default-128"}
    # tile_of() = 1 with several tiles in the weight and in the data gradient; NT = 8 twice
    assert bwd["g2x4_32_48_s13"]["few"]["wgrad"][:2] == (1, 3) and bwd["g1x3_48_32_s11"]["few"]["dgrad"] == ("mfma", 1, 3)
    assert bwd["g1x9_128_256_s11"]["few"]["wgrad"][:2] == (8, 2)
    assert {bwd[n]["few"]["wgrad"][0] for n in bwd} == {1, 2, 4, 8}
    # kw = 1 at cin = 16: the 16-tap fragments exist and no strip kernel matches
    assert G.has_pad16_fragments(by["g4x1_16_16_s21"]) and G.strip_kernel(by["g4x1_16_16_s21"], 3) is None
    # 3. s_conv1 off [2, 2]: ovn_absmax_forward, the generic kernel, then the s_conv2 strip; batches above SMALL_NB switch kernels
    for (strides, a3), (h, w) in list(G.SMALL.items()) + [(G.DOCUMENTED[:2], G.DOCUMENTED[2])]:
        layers = WT.leg_layers(4, G.cfg_of(strides, a3, (h, w), 0))
        for nb in (1, 2, 6):
            path, absmax = G.leg_path_f16x3(layers, nb, h, w)
            k = dict(path)
            assert absmax and k["s_conv1"] == "conv_mfma_f16x3_kernel" and k["s_conv2"] == "conv_strip_small_kernel", (strides, a3)
            mid = "conv_strip_kernel<NTW=1>" if nb <= G.SMALL_NB else "conv_strip_kernel<NTW=2>"
            assert k["s_conv3"] == k["s_conv4"] == mid and (not a3 or k["s_conv3a"] == mid)
            assert all(k["s_conv%d" % i] == "conv_strip_kernel<NTW=1>" for i in range(5, 11))
        assert G.forward_f16x3(layers[0], 2, h, w)["gather"] == "vec4"
        assert G.backward(layers[0], 1, h, w)["dgrad"] == ("plain",)
    shipped, absmax = G.leg_path_f16x3(WT.leg_layers(4, S.REFERENCE_MODEL_CFG), 2, 64, 900)
    assert not absmax and "conv_mfma_f16x3_kernel" not in dict(shipped).values()
    assert [k for _, k in shipped] == ["leg_front"] * 2 + ["conv_strip_kernel<NTW=1>"] * 3 + ["leg_tail"] * 6
    # 4. the strip layers on both sides of the tile choice, and what the bit-identity cases compare
    assert [l.kw for l in G.STRIP_LAYERS] == [9, 7, 5, 3]
    for l in G.STRIP_LAYERS:
        for ow, want in G.STRIP_WIDTHS.items():
            assert G.strip_tile(ow) == want, (l.name, ow)
            assert G.forward_f16x3(l, 2, 1, ow + l.kw - 1)["kernel"] == "conv_strip_kernel<NTW=1>"
        generic = G.forward_f16x3(l, 2, 1, 160 + l.kw - 1, aligned=False)
        assert generic["kernel"] == "conv_mfma_f16x3_kernel" and generic["gather"] == "scalar"
    assert {(tw, pad > 0) for tw, pad in G.STRIP_WIDTHS.values()} == {(80, False), (80, True), (96, False), (96, True)}
    assert G.strip_tile(160) == (80, 0) and G.pad_rows(160, 96) == 32 and G.strip_tile(81)[0] != G.strip_tile(80)[0]
    assert tuple(G.S_CONV3[1:7]) == (3, 15, 32, 64, 2, 1)
    assert G.forward_f16x3(G.S_CONV3, 2, 5, 150)["kernel"] == "conv_strip_kernel<NTW=1>"
    assert G.forward_f16x3(G.S_CONV3, 6, 5, 150)["kernel"] == "conv_strip_kernel<NTW=2>"
    assert G.forward_f16x3(G.S_CONV3, 6, 5, 150, aligned=False)["kernel"] == "conv_mfma_f16x3_kernel"
    assert [(l.name, G.out_shape(l, h, w)) for l, h, w in G.STRIP_BITS] == [("s_conv3", (2, 136)), ("s_conv3", (3, 136)),
                                                                           ("s_conv3a", (3, 49)), ("s_conv4", (2, 92))]
    for l, h, w in G.STRIP_BITS:
        assert G.forward_f16x3(l, 2, h, w)["kernel"] == "conv_strip_kernel<NTW=1>"
        assert G.forward_f16x3(l, 6, h, w)["kernel"] == "conv_strip_kernel<NTW=2>"
        assert G.forward_f16x3(l, 6, h, w, aligned=False)["kernel"] == "conv_mfma_f16x3_kernel"
        x2, x6 = G.strip_bits_input(l, h, w, 2), G.strip_bits_input(l, h, w, 6)
        assert x6.shape == (6, h, w, l.cin) and np.array_equal(x6[:2], x2)
    assert [(l.name, G.out_shape(l, h, w)) for l, h, w in G.FRONT_ALONE] == [("s_conv1", (5, 23)), ("s_conv2", (3, 46))]
    assert all(G.strip_kernel(l, nb) == "conv_strip_small_kernel" for l, _, _ in G.FRONT_ALONE for nb in (1, 3))
    # 5. fewer than 128 output positions per image
    l = G.SMALL_LAYER
    assert G.out_shape(l, 11, 13) == (5, 5) and G.forward_f16x3(l, 1, 11, 13)["kernel"] == "refused"
    assert G.out_shape(l, l.kh, l.kw) == (1, 1) and G.forward_f16x3(l, 1, l.kh, l.kw)["kernel"] == "refused"
    f = G.FINALIZE_LAYER                                               # the whole-leg form of the rule (ovn_finalize)
    assert G.strip_kernel(f, 2) is None and f.cout == 128 and G.out_shape(f, 1, 128) == (1, 127) and WT.FEAT_W_MIN <= 127 <= WT.FEAT_W_MAX
    assert G.leg_path_f16x3([f], 2, 1, 128)[0] == [(f.name, "refused")]
    assert G.leg_path_f16x3([f], 2, 1, 129)[0] == [(f.name, "conv_mfma_f16x3_kernel")]


def _alive64(l, w, x):
    out, _ = L.conv_layer(torch.tensor(x, dtype=torch.float64), torch.tensor(w[l.name + "/kernel"], dtype=torch.float64),
                          torch.tensor(w[l.name + "/bias"], dtype=torch.float64), (l.sh, l.sw))
    return float((out > 0).double().mean())


@pytest.mark.parametrize("l", G.SYNTH, ids=G.SYNTH_IDS)
def test_synthetic_layers_alive_and_float32_inside_the_bound(l):
    w = G.layer_weights(l)
    x = G.forward_input(l)
    ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (l.sh, l.sw))
    assert 0.2 < float((ref > 0).mean()) < 0.8
    assert np.array_equal(x[1], np.float32(300) * x[0])
    out32, _ = L.conv_layer(torch.tensor(x), torch.tensor(w[l.name + "/kernel"]), torch.tensor(w[l.name + "/bias"]), (l.sh, l.sw))
    rt = E.ratio(out32.numpy(), ref, B["f32"])
    assert rt <= 1.0, (l.name, rt)
    assert np.all(B["f16x3"] >= B["f32"])
    for which in ("few", "odd", "long"):
        xb, _ = G.backward_data(0, l, which)
        assert 0.2 < _alive64(l, w, xb) < 0.8, (l.name, which)


@pytest.mark.parametrize("case", list(G.SMALL), ids=G.SMALL_IDS)
def test_first_layer_and_whole_leg_fixtures_alive(case):
    strides, a3 = case
    cfg = G.small_cfg(strides, a3)
    h, wi = G.SMALL[case]
    w = L.leg_weights(4, cfg, seed=0, feat_w=45)
    l = WT.leg_layers(4, cfg)[0]
    for which in ("few", "odd", "long"):
        xb, _ = G.backward_data(0, l, which)
        assert 0.2 < _alive64(l, w, xb) < 0.8, (case, which)
    if case in G.BACKWARD:                       # the fixture of `_whole_leg`: its last layer is neither dead nor all alive
        for n in (1, G.SCAN_BLOCK + 1):
            rng = np.random.default_rng([45, n, 5])
            weights = L.leg_weights(4, cfg, seed=45, feat_w=45)
            images = L.make_images(rng, n, h, wi, 4)
            names = L.leg_names(4, cfg)
            acts = L.leg_forward([torch.tensor(weights[k], dtype=torch.float64) for k in names], torch.tensor(images, dtype=torch.float64),
                                 WT.leg_layers(4, cfg))
            assert tuple(acts[-1].shape) == (n, 1, 45, 128)
            assert 0.2 < float((acts[-1] > 0).double().mean()) < 0.8, (case, n)


def test_strip_layers_float32_inside_the_bound():
    w = S.make_test_weights(4, seed=0)
    for l in G.STRIP_LAYERS:
        x = G.strip_input(l, 81)
        ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (1, 1))
        out32, _ = L.conv_layer(torch.tensor(x), torch.tensor(w[l.name + "/kernel"]), torch.tensor(w[l.name + "/bias"]), (1, 1))
        assert ref.shape == (2, 1, 81, 128) and E.ratio(out32.numpy(), ref, B["f32"]) <= 1.0, l.name


def test_strided_layer_gradients_match_central_differences():
    l = G.SYNTH[-1]                                   # (4, 3, 16, 32, 3, 2)
    assert (l.sh, l.sw) == (3, 2)
    rng = np.random.default_rng(5)
    h, w = l.kh + 2 * l.sh + 2, l.kw + 4 * l.sw + 1   # 3 x 5 windows, two uncovered rows and one uncovered column
    x = rng.normal(0, 1, (2, h, w, l.cin))
    k, b = rng.normal(0, 0.3, (l.kh, l.kw, l.cin, l.cout)), rng.normal(0, 0.3, l.cout)

    def run(k_, b_, x_, mask=None):
        return L.conv_layer(torch.tensor(x_), torch.tensor(k_), torch.tensor(b_), (l.sh, l.sw), mask)[0]
    out = run(k, b, x)
    assert tuple(out.shape) == (2, 3, 5, l.cout)
    mask = (out > 0).numpy()
    d = rng.normal(0, 1, out.shape)
    g = L.layer_grads(k, b, x, mask, d, (l.sh, l.sw))
    eps = 1e-6
    for pi, name in enumerate(("dkernel", "dbias", "din")):
        for _ in range(8):
            ps = [k.copy(), b.copy(), x.copy()]
            idx = tuple(int(rng.integers(0, s)) for s in ps[pi].shape)
            if name == "din":
                idx = idx[:1] + (int(rng.integers(0, h - 2)), int(rng.integers(0, w - 1))) + idx[3:]
            hi, lo = [q.copy() for q in ps], [q.copy() for q in ps]
            hi[pi][idx] += eps
            lo[pi][idx] -= eps
            fd = float(((run(*hi, mask) - run(*lo, mask)) * torch.tensor(d)).sum()) / (2 * eps)
            assert abs(fd - float(g[name][idx])) <= 1e-6 * max(1.0, abs(fd)), (name, idx, fd, float(g[name][idx]))
    assert np.all(g["din"][:, -2:] == 0) and np.all(g["din"][:, :, -1] == 0)
    assert np.all(np.any(g["din"][:, :-2] != 0, axis=(0, 2, 3))) and np.all(np.any(g["din"][:, :, :-1] != 0, axis=(0, 1, 3)))


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    assert lib.ovn_add_leg_layer(None, b"x", None, None, 3, 5, 16, 32, 2, 2, None) == 1
    assert b"NULL argument" in lib.ovn_last_error()
    assert lib.ovn_debug_conv(None, 0, None, 1, 8, 32, None, None) == 1
    assert lib.ovn_debug_conv_grad(None, 0, None, None, None, 1, 8, 32, None, None, None, None) == 1
    assert lib.ovn_finalize(None, None) == 1
    assert lib.ovn_leg_forward_train(None, None, 1, None, None) == 1
    assert lib.ovn_leg_backward(None, None, None, 1, None, None, 0, None) == 1
    assert lib.ovn_leg(None, None, 1, None, None) != 0
    assert lib.ovn_set_leg_precision(None, 0) != 0


def test_the_documents_state_the_128_position_rule():
    header = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    comment = header[:header.index("int ovn_add_leg_layer(")]
    comment = " ".join(comment[-3000:].replace("\n *", " ").split())
    assert "fewer than 128 output positions" in comment and "ovn_finalize" in comment
    assert "128 output positions" in " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
