"""GPU (MI355X): the leg off its eleven shipped layers -- every `strides_layer1`, single layers of any geometry the C ABI accepts,
and the 1 x KW strip layers on both sides of their tile choice -- against the project's own references: the elementwise fp64 bounds
of oracle/error_bounds.py (`leg_with_bounds`, `leg_layer_bound`; err / bound <= 1 passes, in 'f16x3' and 'f32') and, for the
backward pass, the rule of tests/test_gpu_leg_train.py (the GPU's ReLU masks forced into tests/_leg_grad_ref.py, every tensor
within 4 T of fp64, T the error of the float32 CPU restatement).  The cases, their inputs and the host-side mirror of the dispatch
that says which kernel each one reaches are in tests/_leg_geometry_ref.py; tests/test_leg_geometry_host.py guards them on the host.
Every test prints its worst err / bound or err / T.

  1. `strides_layer1` [1, 1], [1, 2], [2, 1], with and without `additional_unsymmetric_layer3a`, at the smallest input that gives
     1 x 45, and INTEGRATION.md's 16 x 900 with [1, 2] -> 1 x 371.  There s_conv1 leaves the fused front kernels: ovn_absmax_forward,
     the generic f16x3 kernel with per-row scales, then the s_conv2 strip fed by the generic kernel's maxima.
       whole leg and every layer alone against the bounds; a scan alone, in a batch of 6 (the batched configuration of
       conv_strip_kernel instead of the narrow one for s_conv3 / 3a / 4) and next to a scan scaled by 300: the same bits; the training forward's last block
       bitwise `engine.leg` under 'f32'; s_conv1 alone through ovn_debug_conv_grad ('few', 'odd', 'long'; with a row stride of 1
       every input row gets a gradient); the whole leg's backward pass at n = 1 and n = scan block + 1; `Infer` on 16 x 247.
  2. Single layers (kh, kw, cin, cout, sh, sw) registered alone through ovn_add_leg_layer: forward on three scans of 8 x 17 output
     pixels (M tiles span two scans, scan 1 = 300 x scan 0) in both precisions, backward on 'few' / 'odd' / 'long'.  Fewer than
     128 output positions: 'f32' runs, 'f16x3' returns OVN_ERR_ARG and leaves the output untouched; for a context's own input
     size ovn_finalize refuses in f16x3, so ovn_leg never meets the rule.  Registration refusals.  The shipped s_conv1 / s_conv2
     alone (conv_strip_small_kernel, which the fused front kernel keeps the shipped leg away from) with a row block past the image.
  3. s_conv5 / 8 / 9 / 10 alone at output widths 80, 81, 96, 97, 160 (80- and 96-pixel tiles, exact and padded) against the bound;
     at 160, and for s_conv3 / s_conv3a / s_conv4 at nb = 2 and nb = 6 (full and partial row blocks and tiles), the strip kernel's
     output is BITWISE the generic kernel's (the same layer on a view of the input 4 bytes into an allocation, which
     ovn_conv_strip_try declines): conv_strip_kernel in its narrow (one n-tile per wave) and batched (two n-tiles per wave, two
     rows per workgroup) configurations and conv_mfma_f16x3_kernel give the same bits, which is what batch independence rests on."""
import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd import weights as WT
from tests import _leg_geometry_ref as G
from tests import _leg_grad_ref as L
from tests.test_gpu_leg_train import _check_layer, _engine, _whole_leg
from tests.test_gpu_width_edges import infer_end_to_end, leg_against_the_bound
from tools import synthetic as S

pytestmark = pytest.mark.gpu

SB = L.SCAN_BLOCK
CASES = list(G.SMALL)


def _tag(case):
    return "strides %s%s" % (list(case[0]), " 3a" if case[1] else "")


@pytest.fixture(scope="module")
def legs():
    """case -> (engine, weights) with the weights of the backward fixtures, built on first use."""
    made = {}

    def get(case):
        if case not in made:
            cfg = G.small_cfg(*case)
            w = L.leg_weights(4, cfg, seed=0, feat_w=45)
            made[case] = (_engine(*G.SMALL[case], 4, w, cfg), w)
        return made[case]
    yield get
    for e, _ in made.values():
        e.close()


@pytest.fixture(scope="module")
def layer_engines():
    made = {}

    def get(l):
        if l.name not in made:
            w = G.layer_weights(l)
            made[l.name] = (G.LayerEngine(l, w), w)
        return made[l.name]
    yield get
    for e, _ in made.values():
        e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. every strides_layer1 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=G.SMALL_IDS)
def test_leg_and_every_layer_against_the_bound(case):
    h, wi = G.SMALL[case]
    leg_against_the_bound(G.small_cfg(*case), h, wi, 45, _tag(case))


def test_documented_16_beam_leg_against_the_bound():
    strides, a3, (h, wi), fw = G.DOCUMENTED
    leg_against_the_bound(G.cfg_of(strides, a3, (h, wi), fw), h, wi, fw, _tag((strides, a3)), layers=("s_conv1",))


@pytest.mark.parametrize("case", CASES, ids=G.SMALL_IDS)
def test_batch_independence_and_training_forward(case, legs):
    eng, _ = legs(case)
    h, wi = G.SMALL[case]
    rng = np.random.default_rng([h, wi, 6])
    a = _dev(rng.normal(0.5, 1.0, size=(6, h, wi, 4)).astype(np.float32))
    big = (300 * a[:1]).contiguous()
    try:
        eng.set_leg_precision("f16x3")
        one = eng.leg(a[1:2].contiguous())
        assert torch.isfinite(one).all() and float(one.max()) > 0
        assert torch.equal(eng.leg(a)[1:2], one), "in a batch of 6"
        assert torch.equal(eng.leg(torch.cat([a[1:2], big]).contiguous())[:1], one), "before a scan scaled by 300"
        assert torch.equal(eng.leg(torch.cat([big, a[1:2]]).contiguous())[1:], one), "after a scan scaled by 300"
        acts = eng.leg_forward_train(a[:2].contiguous())              # fp32 whatever the mode says
        eng.set_leg_precision("f32")
        assert torch.equal(acts[-1].view(2, 45, 128), eng.leg(a[:2].contiguous()))
    finally:
        eng.set_leg_precision("f32")


@pytest.mark.parametrize("which", ("few", "odd", "long"))
@pytest.mark.parametrize("case", CASES, ids=G.SMALL_IDS)
def test_first_layer_alone_backward(case, which, legs):
    eng, w = legs(case)
    l = WT.leg_layers(4, G.small_cfg(*case))[0]
    assert (l.sh, l.sw) == case[0] and l.cin % 16 != 0
    _check_layer(eng, w, 0, l, which, "s_conv1 %s %s" % (_tag(case), which))      # with sh = 1 it asserts a gradient in every row


@pytest.mark.parametrize("n", (1, SB + 1))
@pytest.mark.parametrize("case", G.BACKWARD, ids=[G.SMALL_IDS[CASES.index(c)] for c in G.BACKWARD])
def test_whole_leg_backward(case, n):
    h, wi = G.SMALL[case]
    _whole_leg(G.small_cfg(*case), h, wi, 45, n, "leg %s n%d" % (_tag(case), n))


def test_infer_on_a_16_beam_sensor(tmp_path, fixture_npz):
    case = ((1, 2), False)
    h, wi = G.SMALL[case]
    assert (h, wi) == (16, 247)
    infer_end_to_end(tmp_path, fixture_npz, G.small_cfg(*case), h, wi, 45)


# ---- 2. single layers the C ABI accepts ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l", G.SYNTH, ids=G.SYNTH_IDS)
def test_single_layer_forward(l, layer_engines):
    le, w = layer_engines(l)
    x = G.forward_input(l)
    oh, ow, _, _ = G.forward_shape(l)
    ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (l.sh, l.sw))
    xt = _dev(x)
    try:
        for mode in ("f16x3", "f32"):
            le.set_leg_precision(mode)
            out = le.debug_conv(0, xt).cpu().numpy()
            assert out.shape == (3, oh, ow, l.cout)
            rt = E.ratio(out, ref, B[mode])
            print("\n[layer %s %s] worst err / bound: %.3g" % (l.name, mode, rt))
            assert rt <= 1.0, (l.name, mode, rt)
    finally:
        le.set_leg_precision("f32")


@pytest.mark.parametrize("l,h,wi", G.FRONT_ALONE, ids=[c[0].name for c in G.FRONT_ALONE])
def test_front_layers_alone_forward(l, h, wi):
    """The shipped s_conv1 (C = 4) and s_conv2 registered alone: conv_strip_small_kernel (s_conv1: scaled by its strip's own maximum),
    with a last row block that reaches past the image, against the f16x3 bound; a scan alone has the bits it has in the batch.
    (Not compared with the generic kernel: the K chunks are laid out differently, taps padded to 16, and s_conv1 scales by its
    strip's maximum, so equal bits are not claimed.)"""
    w = S.make_test_weights(4, seed=0)
    le = G.LayerEngine(l, w)
    try:
        le.set_leg_precision("f16x3")
        x = G.front_alone_input(l, h, wi)
        ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (l.sh, l.sw), modes=("f16x3",))
        xt = _dev(x)
        out = le.debug_conv(0, xt)
        rt = E.ratio(out.cpu().numpy(), ref, B["f16x3"])
        print("\n[%s alone %dx%d f16x3] worst err / bound: %.3g" % (l.name, h, wi, rt))
        assert out.shape == (3,) + G.out_shape(l, h, wi) + (l.cout,) and rt <= 1.0, (l.name, rt)
        for i in range(3):
            assert torch.equal(le.debug_conv(0, xt[i:i + 1].contiguous()), out[i:i + 1]), "%s: scan %d alone" % (l.name, i)
    finally:
        le.close()


@pytest.mark.parametrize("which", ("few", "odd", "long"))
@pytest.mark.parametrize("l", G.SYNTH, ids=G.SYNTH_IDS)
def test_single_layer_backward(l, which, layer_engines):
    le, w = layer_engines(l)
    _check_layer(le, w, 0, l, which, "%s %s" % (l.name, which))


def test_fewer_than_128_output_positions(layer_engines):
    l = G.SMALL_LAYER
    le, w = layer_engines(l)
    rng = np.random.default_rng(128)
    try:
        for h, wi in ((11, 13), (l.kh, l.kw)):                       # 5 x 5 and 1 x 1 output positions
            x = rng.normal(0.0, 1.0, (2, h, wi, l.cin)).astype(np.float32)
            ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (l.sh, l.sw), modes=("f32",))
            xt = _dev(x)
            le.set_leg_precision("f32")
            out = le.debug_conv(0, xt).cpu().numpy()
            rt = E.ratio(out, ref, B["f32"])
            print("\n[layer %s %dx%d f32] worst err / bound: %.3g" % (l.name, h, wi, rt))
            assert out.shape == ref.shape and rt <= 1.0
            le.set_leg_precision("f16x3")
            nan = torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda")
            assert le.conv_rc(xt, nan) == 1
            msg = le.lib.ovn_last_error()
            assert b"fewer than 128 output positions" in msg and l.name.encode() in msg
            assert bool(torch.isnan(nan).all()), "the refused call wrote to its output"
    finally:
        le.set_leg_precision("f32")


def test_finalize_refuses_what_f16x3_cannot_serve():
    """A leg whose context input gives a generic-kernel layer fewer than 128 positions: refused by ovn_finalize in f16x3 and by a
    later switch to f16x3, never met by ovn_leg; it runs in f32.  One column more and f16x3 takes it."""
    import ctypes as C
    from overlapnet_amd.engine import _ptr
    l = G.FINALIZE_LAYER                                               # (1, 2, 128, 128, 1, 1): no strip kernel has kw = 2
    w = G.layer_weights(l)
    rng = np.random.default_rng(127)
    for wi, served in ((128, False), (129, True)):                     # 127 / 128 output positions
        le = G.LayerEngine(l, w, in_h=1, in_w=wi)
        try:
            h, lib, fw = le.eng._h, le.lib, C.c_int(0)
            x = np.maximum(rng.normal(0.2, 1.0, (2, 1, wi, 128)), 0).astype(np.float32)
            ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (1, 1))
            out = torch.full((2, wi - 1, 128), float("nan"), dtype=torch.float32, device="cuda")
            modes = ("f16x3", "f32")
            if not served:
                assert lib.ovn_finalize(h, C.byref(fw)) == 1
                msg = lib.ovn_last_error()
                assert b"fewer than 128 output positions" in msg and l.name.encode() in msg and fw.value == 0
                assert lib.ovn_leg(h, _ptr(_dev(x)), 2, _ptr(out), le.eng._stream()) == 3        # still not finalized
                le.set_leg_precision("f32")
                modes = ("f32",)
            assert lib.ovn_finalize(h, C.byref(fw)) == 0 and fw.value == wi - 1
            if not served:
                assert lib.ovn_set_leg_precision(h, 1) == 1 and b"fewer than 128 output positions" in lib.ovn_last_error()
            for mode in modes:
                if served:
                    le.set_leg_precision(mode)
                out.fill_(float("nan"))
                assert lib.ovn_leg(h, _ptr(_dev(x)), 2, _ptr(out), le.eng._stream()) == 0, lib.ovn_last_error()
                torch.cuda.synchronize()
                rt = E.ratio(out.cpu().numpy().reshape(ref.shape), ref, B[mode])
                print("\n[leg of %s alone, 1x%d %s] worst err / bound: %.3g" % (l.name, wi, mode, rt))
                assert rt <= 1.0, (wi, mode, rt)
        finally:
            le.close()


def test_registration_refusals():
    l = G.SMALL_LAYER
    w = G.layer_weights(l)
    le = G.LayerEngine(l, w)
    dummy_k, dummy_b = np.zeros(65536, np.float32), np.zeros(256, np.float32)
    try:
        bad = [("cout = 24", l._replace(name="bad", cin=32, cout=24), b"multiple of 16"),
               ("kh = 0", l._replace(name="bad", cin=32, kh=0), b"bad geometry"),
               ("kw = 0", l._replace(name="bad", cin=32, kw=0), b"bad geometry"),
               ("sh = 0", l._replace(name="bad", cin=32, sh=0), b"bad geometry"),
               ("sw = 0", l._replace(name="bad", cin=32, sw=0), b"bad geometry"),
               ("cin of another layer", l._replace(name="bad", cin=16), b"previous layer produces 32")]
        for what, spec, text in bad:
            assert le.add(spec, dummy_k, dummy_b) == 1, what
            assert text in le.lib.ovn_last_error(), (what, le.lib.ovn_last_error())
        nxt = G.SYNTH[1]                                               # (2, 4, 32, 48, 1, 3): takes the 32 channels of the first
        wn = G.layer_weights(nxt)
        assert le.add(nxt, wn[nxt.name + "/kernel"], wn[nxt.name + "/bias"]) == 0, le.lib.ovn_last_error()
        x = G.forward_input(nxt)
        ref, B = E.leg_layer_bound(x, wn[nxt.name + "/kernel"], wn[nxt.name + "/bias"], (nxt.sh, nxt.sw), modes=("f32",))
        le.set_leg_precision("f32")
        out = torch.full(ref.shape, float("nan"), dtype=torch.float32, device="cuda")
        assert le.conv_rc(_dev(x), out, layer=1) == 0
        assert E.ratio(out.cpu().numpy(), ref, B["f32"]) <= 1.0
        assert le.conv_rc(_dev(x), out, layer=2) == 1                  # the refused layers were not registered
    finally:
        le.close()


# ---- 3. the strip tile choice and the bit-identity claim ------------------------------------------------------------------------------

def _off4(x):
    """The same values on a view that starts 4 bytes into an allocation: ovn_conv_strip_try declines it."""
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _strip_layer(l):
    w = S.make_test_weights(4, seed=0, model_cfg=G.CFG_3A if l.name == "s_conv3a" else None)
    return G.LayerEngine(l, w), w


@pytest.mark.parametrize("l", G.STRIP_LAYERS, ids=[l.name for l in G.STRIP_LAYERS])
def test_strip_tile_choice(l):
    le, w = _strip_layer(l)
    try:
        le.set_leg_precision("f16x3")
        for ow, (tw, pad) in G.STRIP_WIDTHS.items():
            x = G.strip_input(l, ow)
            assert x.shape == (2, 1, ow + l.kw - 1, 128)
            ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (1, 1), modes=("f16x3",))
            xt = _dev(x)
            out = le.debug_conv(0, xt)
            rt = E.ratio(out.cpu().numpy(), ref, B["f16x3"])
            print("\n[%s ow %d: tile %d, %d padded] worst err / bound: %.3g" % (l.name, ow, tw, pad, rt))
            assert out.shape == (2, 1, ow, 128) and rt <= 1.0, (l.name, ow, rt)
            if ow == 160:
                generic = le.debug_conv(0, _off4(xt))
                assert torch.equal(generic, out), "%s: the strip kernel and the generic kernel differ" % l.name
    finally:
        le.close()


@pytest.mark.parametrize("nb", (2, 6))
def test_strip_kernels_give_the_generic_kernels_bits(nb):
    """Every input of G.STRIP_BITS (s_conv3 on 5 x 150 and 7 x 150, s_conv3a on 7 x 60, s_conv4 on 4 x 100): the narrow (nb = 2) and
    the batched (nb = 6) configuration of conv_strip_kernel against the fp64 bound and, bitwise, against conv_mfma_f16x3_kernel;
    scans 0 and 1 of the nb = 6 call have the bits of the nb = 2 call (narrow = batched)."""
    for l, h, wi in G.STRIP_BITS:
        le, w = _strip_layer(l)
        tag = "%s %dx%d nb %d" % (l.name, h, wi, nb)
        try:
            le.set_leg_precision("f16x3")
            x = G.strip_bits_input(l, h, wi, nb)
            assert x.shape == (nb, h, wi, l.cin)
            ref, B = E.leg_layer_bound(x, w[l.name + "/kernel"], w[l.name + "/bias"], (l.sh, l.sw), modes=("f16x3",))
            xt = _dev(x)
            out = le.debug_conv(0, xt)
            rt = E.ratio(out.cpu().numpy(), ref, B["f16x3"])
            print("\n[%s] worst err / bound: %.3g" % (tag, rt))
            assert out.shape == (nb,) + G.out_shape(l, h, wi) + (l.cout,) and rt <= 1.0, (tag, rt)
            generic = le.debug_conv(0, _off4(xt))
            rg = E.ratio(generic.cpu().numpy(), ref, B["f16x3"])
            print("[%s, generic kernel] worst err / bound: %.3g" % (tag, rg))
            assert rg <= 1.0, (tag, rg)
            assert torch.equal(generic, out), "%s: the strip kernel and the generic kernel differ" % tag
            if nb > G.SMALL_NB:
                narrow = le.debug_conv(0, xt[:2].contiguous())
                assert torch.equal(out[:2], narrow), "%s: the batched and the narrow configuration differ" % tag
        finally:
            le.close()
