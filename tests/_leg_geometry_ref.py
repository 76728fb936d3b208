"""TEST INFRASTRUCTURE: the leg geometries off the shipped eleven layers that tests/test_gpu_leg_geometry.py runs on the GPU and
tests/test_leg_geometry_host.py guards on the host -- the table of cases, their seeded inputs and weights, a host-side mirror of the
library's kernel dispatch (so that "this case reaches that branch" is an assertion, not a comment), and `LayerEngine`, one layer
registered alone through the C entry points with the interface of `OvnEngine.debug_conv` / `debug_conv_grad`.

  SMALL        every `strides_layer1` other than [2, 2], with and without `additional_unsymmetric_layer3a`, at the smallest input that
               gives a 1 x 45 feature volume; DOCUMENTED is INTEGRATION.md's 16 x 900 with [1, 2] -> 1 x 371.
  SYNTH        single layers the C ABI accepts (kh, kw, cin, cout, sh, sw) and the shipped table never produces.
  STRIP_WIDTHS output widths of the 1 x KW strip layers on both sides of the 80- / 96-pixel tile choice.

The mirror restates, in Python, the `if`s of ovn_conv_forward_f16x3 / ovn_conv_strip_try (csrc/conv_f16x3.hip, conv_strip.hip),
ovn_conv_forward (conv_f32.hip), ovn_leg (ovn_api.hip) and ovn_leg_layer_backward (leg_backward.hip)."""
import numpy as np

from overlapnet_amd import weights as WT
from overlapnet_amd.weights import ConvSpec
from tests import _leg_grad_ref as L
from tools import synthetic as S

SCAN_BLOCK = L.SCAN_BLOCK
SMALL_NB = 4                 # conv_strip.hip: calls of at most this many scans take the narrow configuration of conv_strip_kernel (one
                             # n-tile per wave, NTW = 1), larger ones the batched one (NTW = 2)
STRIP_NARROW, STRIP_BATCHED = "conv_strip_kernel<NTW=1>", "conv_strip_kernel<NTW=2>"
MIN_POSITIONS = 128          # conv_f16x3.hip: the generic f16x3 kernel needs this many output positions per image
FEAT_W_TAIL = 360            # leg_tail.hip: the fused tail runs 360-column volumes only

# (strides_layer1, additional_unsymmetric_layer3a) -> the smallest (H, W) input whose feature volume is 1 x 45
SMALL = {((1, 1), False): (16, 131), ((1, 1), True): (32, 142),
         ((1, 2), False): (16, 247), ((1, 2), True): (32, 269),
         ((2, 1), False): (32, 131), ((2, 1), True): (64, 142)}
SMALL_IDS = ["s%d%d%s" % (s[0], s[1], "-3a" if a3 else "") for s, a3 in SMALL]
DOCUMENTED = ((1, 2), False, (16, 900), 371)        # INTEGRATION.md, "Input shape and feature width"
BACKWARD = [((1, 1), False), ((1, 2), False), ((1, 2), True)]      # whole-leg backward cases


def cfg_of(strides, a3, hw, fw):
    return dict(S.REFERENCE_MODEL_CFG, inputShape=list(hw), leg_output_width=fw, strides_layer1=list(strides),
                additional_unsymmetric_layer3a=bool(a3))


def small_cfg(strides, a3):
    return cfg_of(strides, a3, SMALL[(strides, a3)], 45)


def _spec(kh, kw, cin, cout, sh, sw):
    return ConvSpec("g%dx%d_%d_%d_s%d%d" % (kh, kw, cin, cout, sh, sw), kh, kw, cin, cout, sh, sw, True)


# what each reaches is asserted by tests/test_leg_geometry_host.py::test_dispatch_mirror_reaches_every_branch
SYNTH = [_spec(*g) for g in (
    (3, 5, 16, 32, 2, 2),      # MFMA data gradient with a column and a row stride of 2
    (2, 4, 32, 48, 1, 3),      # sw = 3; cout = 48: the default: launch branch with three column blocks, three wgrad tiles of 16
    (1, 3, 48, 32, 1, 1),      # cin = 48: three channel tiles of 16 in the data gradient; K = 144
    (1, 1, 64, 64, 1, 1),      # one tap, KW Cin = 64
    (3, 3, 8, 16, 3, 1),       # cin = 8: 16-byte gather, plain data gradient; sh = 3; K = 72, KW Cin = 24 < 32 (the while wrap)
    (2, 2, 12, 16, 1, 1),      # cin = 12: a multiple of 4, not of 8; K = 48
    (4, 1, 16, 16, 2, 1),      # kw = 1 at cin = 16: the 16-tap fragments are built and no strip kernel matches
    (1, 9, 128, 256, 1, 1),    # cout = 256: the 128-column tile with two column blocks; wgrad NT = 8 twice
    (4, 3, 16, 32, 3, 2),      # the MFMA data gradient with a row stride of 3 (the table above has sh = 3 only at cin = 8)
)]
SYNTH_IDS = [l.name for l in SYNTH]
SMALL_LAYER = SYNTH[0]       # the layer of the "fewer than 128 output positions" cases
FINALIZE_LAYER = _spec(1, 2, 128, 128, 1, 1)       # a whole "leg" of one layer (1 x W x 128 out) that no strip kernel takes
STRIP_LAYERS = [l for l in WT.leg_layers(4) if l.name in ("s_conv5", "s_conv8", "s_conv9", "s_conv10")]      # kw 9, 7, 5, 3
STRIP_WIDTHS = {80: (80, 0), 81: (96, 15), 96: (96, 0), 97: (80, 63), 160: (80, 0)}       # output width -> (tile, padded pixels)
S_CONV3 = WT.leg_layers(4)[2]
CFG_3A = dict(S.REFERENCE_MODEL_CFG, additional_unsymmetric_layer3a=True)
_BY_NAME = {l.name: l for l in WT.leg_layers(4, CFG_3A)}
# the plane-layout strip layers with a narrow and a batched configuration, on inputs (h, w) of at least 128 output positions (the
# generic kernel takes them too): layer, h, w, then what each input is there for
STRIP_BITS = [(S_CONV3, 5, 150),               # 2 x 136: one full row pair; tiles 96 + 40 batched, 52 + 52 + 32 narrow
              (S_CONV3, 7, 150),               # 3 x 136: the second row block has one row past the image (load and store guards)
              (_BY_NAME["s_conv3a"], 7, 60),   # 3 x 49: batched tiles 48 + 1 (one m-tile, one valid pixel), narrow 32 + 17
              (_BY_NAME["s_conv4"], 4, 100)]   # 2 x 92: batched tiles 80 + 12, narrow 32 + 32 + 28 (fragments read at their own step)
# s_conv1 (C = 4) and s_conv2 registered alone, (h, w): the pixel-major strip kernel, which the fused front kernel keeps the shipped
# leg away from.  5 x 23 output pixels in row blocks of 3 and 3 x 46 in row blocks of 2: the last block has rows past the image
FRONT_ALONE = [(_BY_NAME["s_conv1"], 13, 60), (_BY_NAME["s_conv2"], 7, 60)]


def layer_weights(l, seed=0):
    """{name/kernel, name/bias} of one layer by the recipe of `_leg_grad_ref.leg_weights` (weights.synthetic_weights with a kernel
    gain of 1.4: Glorot-uniform kernels, biases uniform in +-0.05)."""
    rng = np.random.default_rng([seed, l.kh, l.kw, l.cin, l.cout])
    k = (WT._glorot_uniform(rng, (l.kh, l.kw, l.cin, l.cout)) * np.float32(1.4)).astype(np.float32)
    return {l.name + "/kernel": k, l.name + "/bias": rng.uniform(-0.05, 0.05, size=(l.cout,)).astype(np.float32)}


def forward_shape(l):
    """(oh, ow, h, w) of the forward input: 8 x 17 output pixels (1 x 136 at cin = 128) from an input with sh - 1 rows and sw - 1
    columns more than the windows cover."""
    oh, ow = (1, 136) if l.cin == 128 else (8, 17)
    return oh, ow, (oh - 1) * l.sh + l.kh + l.sh - 1, (ow - 1) * l.sw + l.kw + l.sw - 1


def forward_input(l):
    """Three scans; scan 1 is scan 0 times 300, so that adjacent rows of an M tile carry different f16x3 scales (136 positions per
    scan are no multiple of 16: a tile spans two scans)."""
    _, _, h, w = forward_shape(l)
    rng = np.random.default_rng([7, l.kh, l.kw, l.cin, l.cout, l.sh, l.sw])
    x = rng.normal(0.0, 1.0, (3, h, w, l.cin)).astype(np.float32)
    x[1] = np.float32(300.0) * x[0]
    return x


def strip_bits_input(l, h, w, nb):
    """nb = 2: two scans, scan 1 scaled by 300 (per-scan scales); nb = 6: the same two followed by four more."""
    x = strip_input(l, w - l.kw + 1, nb=2, h=h)
    x[1] *= np.float32(300.0)
    return x if nb == 2 else np.concatenate([x, strip_input(l, w - l.kw + 1, nb=nb - 2, h=h)])


def front_alone_input(l, h, w):
    """Three scans; scan 1 is scan 0 times 300."""
    rng = np.random.default_rng([13, l.kh, l.kw, l.cin, h, w])
    x = rng.normal(0.0, 1.0, (3, h, w, l.cin)).astype(np.float32)
    x[1] = np.float32(300.0) * x[0]
    return x


def strip_input(l, ow, nb=2, h=1):
    rng = np.random.default_rng([11, l.kw, ow, nb, h])
    return np.maximum(rng.normal(0.2, 1.0, (nb, h, ow + l.kw - 1, l.cin)), 0).astype(np.float32)      # a ReLU output, as in the leg


# ---- the dispatch, mirrored ---------------------------------------------------------------------------------------------------------

def out_shape(l, h, w):
    return (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1


def pad_rows(ow, tw):
    return -(-ow // tw) * tw - ow


def strip_tile(ow):
    """(tile, padded pixels) of a 1 x KW, 128 -> 128 strip layer with `ow` output pixels per row (ovn_conv_strip_try)."""
    tw = 80 if pad_rows(ow, 80) <= pad_rows(ow, 96) else 96
    return tw, pad_rows(ow, tw)


def has_pad16_fragments(l):
    return l.cin in (4, 16) and l.kw <= 16           # ovn_conv_prepare_f16x3: wp_h16


def strip_kernel(l, nb, aligned=True):
    """Name of the strip kernel (for the plane-layout kernel: and which of its two kinds of configuration) ovn_conv_strip_try runs
    for this layer, or None when it declines: the rows of STRIP_ROWS in conv_strip.hip."""
    if not aligned:
        return None
    g = (l.kh, l.kw, l.cin, l.cout, l.sh, l.sw)
    if has_pad16_fragments(l):
        return "conv_strip_small_kernel" if g in ((5, 15, 4, 16, 2, 2), (3, 15, 16, 32, 2, 1)) else None
    if l.sw != 1 or (l.kh > 1 and l.sh != 2) or (l.kh == 1 and l.sh != 1):
        return None
    if g[:4] in ((3, 15, 32, 64), (3, 12, 64, 64), (2, 9, 64, 128)):
        return STRIP_NARROW if nb <= SMALL_NB else STRIP_BATCHED
    if g[:4] in ((1, 9, 128, 128), (1, 7, 128, 128), (1, 5, 128, 128), (1, 3, 128, 128)):
        return STRIP_NARROW
    return None


def generic_tile(l, m, f16x3=True):
    """(WM, WN, WAVES_M, WAVES_N, column blocks, branch) of launch_conv_b / launch_conv for `m` output rows."""
    if l.cout in (16, 32, 64):
        t, branch = {16: (2, 1, 4, 1), 32: (2, 2, 4, 1), 64: (2, 4, 4, 1)}[l.cout], "case"
    elif l.cout % 128 == 0:
        t, branch = ((2, 4, 4, 2) if f16x3 and m >= 32 * 1024 else (2, 4, 2, 2)), "default-128"
    else:
        t, branch = (2, 1, 4, 1), "default-16"
    return t + (l.cout // (16 * t[1] * t[3]), branch)


def forward_f16x3(l, nb, h, w, aligned=True):
    """What ovn_conv_forward_f16x3 does with this call -> dict(kernel=..., and for the generic kernel gather / wrap / tile)."""
    k = strip_kernel(l, nb, aligned)
    if k:
        return {"kernel": k}
    oh, ow = out_shape(l, h, w)
    if oh * ow < MIN_POSITIONS:
        return {"kernel": "refused"}
    kwc = l.kw * l.cin
    vec4 = l.cin % 4 == 0 and aligned
    return {"kernel": "conv_mfma_f16x3_kernel", "gather": "vec4" if vec4 else "scalar", "wrap": "select" if kwc >= 32 else "while",
            "tile": generic_tile(l, nb * oh * ow)}


def leg_path_f16x3(layers, nb, h, w):
    """The kernels ovn_leg runs for a batch of nb aligned scans in f16x3, layer by layer: [(layer name, kernel)], and whether the
    first layer's input is scanned by ovn_absmax_forward first."""
    path, li = [], 0
    own = tuple(layers[0][1:7]) == (5, 15, 4, 16, 2, 2)
    while li < len(layers):
        l = layers[li]
        if li == 0 and li + 1 < len(layers) and tuple(l[1:7]) == (5, 15, 4, 16, 2, 2) and tuple(layers[1][1:7]) == (3, 15, 16, 32, 2, 1):
            oh, ow = out_shape(l, h, w)
            if oh >= 3 and ow >= 15:
                path += [(l.name, "leg_front"), (layers[1].name, "leg_front")]
                h, w = out_shape(layers[1], oh, ow)
                li += 2
                continue
        tail = layers[li:]
        if h == 1 and [tuple(t[1:7]) for t in tail] == [(1, kw, 128, 128, 1, 1) for kw in (9, 9, 9, 7, 5, 3)] and w - 36 == FEAT_W_TAIL:
            path += [(t.name, "leg_tail") for t in tail]
            break
        path.append((l.name, forward_f16x3(l, nb, h, w)["kernel"]))
        h, w = out_shape(l, h, w)
        li += 1
    return path, not own


def tile_of(c16):
    return 8 if c16 % 8 == 0 else 4 if c16 % 4 == 0 else 2 if c16 % 2 == 0 else 1


def piece_of(out_px):
    return 256 * min(8, max(1, (SCAN_BLOCK * out_px) // (16 * 256)))


def backward(l, nb, h, w):
    """ovn_leg_layer_backward's launches: wgrad (NT, column tiles, k tiles), dgrad ('mfma', NT, channel tiles) or ('plain',),
    reduction pieces per scan block and scan blocks."""
    oh, ow = out_shape(l, h, w)
    nt = tile_of(l.cout // 16)
    k = l.kh * l.kw * l.cin
    if l.cin % 16 == 0:
        dnt = tile_of(l.cin // 16)
        dgrad = ("mfma", dnt, l.cin // (16 * dnt))
    else:
        dgrad = ("plain",)
    return {"wgrad": (nt, l.cout // (16 * nt), -(-k // 64)), "dgrad": dgrad,
            "pieces": -(-SCAN_BLOCK * oh * ow // piece_of(oh * ow)), "blocks": -(-nb // SCAN_BLOCK)}


def layer_inputs(l):
    """name -> (nb, h, w) of the backward inputs of one layer: tests/test_gpu_leg_train.py's three.  'odd' has stride - 1 rows and
    columns more than the windows cover (one where the stride is 2, none where it is 1), whose data gradient must be exactly zero."""
    xr, xc = l.sh - 1, l.sw - 1
    return {"few": (1, l.kh, l.kw + 4 * l.sw), "odd": (SCAN_BLOCK + 1, l.kh + l.sh + xr, l.kw + 36 * l.sw + xc),
            "long": (1, l.kh + l.sh, l.kw + 149 * l.sw)}


def backward_data(li, l, which):
    """The seeded input and output gradient `_check_layer` of tests/test_gpu_leg_train.py feeds layer `l` (index li in its engine)."""
    nb, h, w = layer_inputs(l)[which]
    oh, ow = out_shape(l, h, w)
    rng = np.random.default_rng([li, nb, h, w, l.cin])
    x = rng.normal(0.0, 1.0, (nb, h, w, l.cin)).astype(np.float32)
    dout = rng.normal(0.0, 1.0, (nb, oh, ow, l.cout)).astype(np.float32)
    return x, dout


# ---- one layer alone on the GPU ----------------------------------------------------------------------------------------------------

class LayerEngine(object):
    """One layer registered alone with `ovn_add_leg_layer` on a context that is never finalized (the debug hooks need no finalized
    leg), behind the interface `_check_layer` uses: device, set_leg_precision, debug_conv(0, x), debug_conv_grad(0, x, out, dout)."""

    def __init__(self, l, weights, in_h=64, in_w=900):
        from overlapnet_amd import _lib
        from overlapnet_amd.engine import OvnEngine
        self.spec, self._lib = l, _lib
        self.eng = OvnEngine(in_h, in_w, l.cin)
        self.lib, self.device = self.eng.lib, self.eng.device
        try:
            _lib.check(self.add(l, weights[l.name + "/kernel"], weights[l.name + "/bias"]), "ovn_add_leg_layer(%s)" % l.name)
        except Exception:
            self.close()
            raise

    def add(self, l, kernel, bias):
        """-> the return code of ovn_add_leg_layer."""
        import torch
        from overlapnet_amd.engine import _ptr
        k = torch.from_numpy(np.ascontiguousarray(kernel, np.float32)).to(self.device)
        b = torch.from_numpy(np.ascontiguousarray(bias, np.float32)).to(self.device)
        rc = self.lib.ovn_add_leg_layer(self.eng._h, l.name.encode(), _ptr(k), _ptr(b), l.kh, l.kw, l.cin, l.cout, l.sh, l.sw, self.eng._stream())
        torch.cuda.synchronize(self.device)
        return rc

    def close(self):
        self.eng.close()

    def set_leg_precision(self, mode):
        self.eng.set_leg_precision(mode)

    def conv_rc(self, x, out, layer=0):
        """ovn_debug_conv on device tensors x (nb, h, w, cin) -> out; returns the code."""
        import torch
        from overlapnet_amd.engine import _ptr
        nb, h, w, _ = x.shape
        rc = self.lib.ovn_debug_conv(self.eng._h, layer, _ptr(x), nb, h, w, _ptr(out), self.eng._stream())
        torch.cuda.synchronize(self.device)
        return rc

    def debug_conv(self, layer, x):
        import torch
        l = self.spec
        nb, h, w, _ = x.shape
        out = torch.full((nb,) + out_shape(l, h, w) + (l.cout,), float("nan"), dtype=torch.float32, device=self.device)
        self._lib.check(self.conv_rc(x, out, layer), "ovn_debug_conv")
        return out

    def debug_conv_grad(self, layer, x, out, dout, want=("din", "dkernel", "dbias")):
        import torch
        from overlapnet_amd.engine import _ptr
        l = self.spec
        nb, h, w, _ = x.shape
        r = {}
        if "din" in want:
            r["din"] = torch.full_like(x, float("nan"))
        if "dkernel" in want:
            r["dkernel"] = torch.full((l.kh, l.kw, l.cin, l.cout), float("nan"), dtype=torch.float32, device=self.device)
        if "dbias" in want:
            r["dbias"] = torch.full((l.cout,), float("nan"), dtype=torch.float32, device=self.device)
        self._lib.check(self.lib.ovn_debug_conv_grad(self.eng._h, layer, _ptr(x), _ptr(out), _ptr(dout), nb, h, w, _ptr(r.get("din")),
                                                     _ptr(r.get("dkernel")), _ptr(r.get("dbias")), self.eng._stream()), "ovn_debug_conv_grad")
        torch.cuda.synchronize(self.device)
        return r
