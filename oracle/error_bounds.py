"""Elementwise error bounds for the HIP path -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`head_pair` / `corr_pair` restate the Delta and correlation heads of `overlapnet_oracle` in fp64 NumPy, keeping every stage of
every pair (tests/test_error_bound_power.py pins them to `delta_head_forward` / `correlation_head_forward`), and `leg_with_bounds`
runs the oracle's leg layer by layer.  This module adds, per pair (or scan) and per stage, an ELEMENTWISE bound B derived from
the arithmetic of the HIP kernels, so that a stage passes when

    |gpu - ref| <= B          element by element (no normalisation by the tensor's largest value)

Error model (u = 2^-24, the fp32 unit roundoff).  One contraction of n products y = b + sum_i x_i w_i contributes its own error
    own = u_prod rms + sqrt(n) u (|v| + rms),   rms = sqrt(sum_i (x_i w_i)^2),  v = the value being accumulated
  * u_prod, error of one product from the operand representation (relative, worst case):
      fp32:    u (operands exact; the product's rounding).
      f16x3:   5 * 2^-22.  x (scaled) = hi + lo, hi = fp16_rtz(x) so |x - hi| < 2^-10 |x|, lo = fp16_rne(x - hi) adds <= 2^-21 |x|;
               a weight is split with a round-to-nearest hi, lo adds <= 2^-22 |w|; the dropped lo * lo product is < 2^-21 |x w|.
               Plus an ABSOLUTE floor: scales put a tensor's largest operand at 2^13..2^14 (ovn_pow2_scale_for, clamped at
               2^+-100 in the Delta head) and lo ends at the fp16 subnormal spacing 2^-24, so every operand also carries up to
               2^-25 / scale: 2^-38 of the largest operand of its tensor (per pair in the head), more where the clamp holds (a
               pair of subnormal volumes).  A stage adds 4 2^-25 / scale sum|W| for it (`_floor`).  It decides the bound where
               one pair spans more than ~2^20 (values 1e-6 next to 1e4, 1e30 next to 1).
      bf16x3:  2^-20.  x = a0 + a1 + a2 exactly (truncated bf16 planes: |a1| < 2^-7 |x|, |a2| < 2^-14 |x|); the six kept
               products drop a1 w2 + a2 w1 + a2 w2 < (2 * 2^-21 + 2^-28) |x w|.
    The per-product errors have independent signs across i, so they add like a random walk: u_prod rms.
  * sqrt(n) u (|v| + rms): the fp32 accumulation.  n roundings, each at most u times a partial sum; a partial sum of terms with
    root-sum-square rms stays within |v| + rms of zero up to O(1) factors, and independent rounding errors add like a random walk.
  * The min form (f16x3 and bf16x3 c_conv1): |l - r| = l' + r' - 2 min(l', r'), l' = l + c, r' = r + c, c = -min(0, smallest value
    of the pair).  Its three terms cancel, so rms and v of c_conv1 are those of the three terms (l'^2 + r'^2 + 4 min^2 under
    W1^2; |b1| + |l' Ws| + |r' W1| + 2 |min W1|), not those of |l - r|.  fp32 mode and the generic path form |l - r| exactly.
  * Carried errors: an input error of size sigma_in reaches the output as sum_i w_i d_i; independent errors of different dot
    products add in quadrature, so sigma_k^2 = own_k^2 + conv(W_k^2, sigma_{k-1}^2).  ReLU is 1-Lipschitz.
  * B = SAFETY sigma with SAFETY = 6, fixed: sigma is already an upper bound of a standard deviation (worst-case u_prod, partial
    sums bounded by |v| + rms); six of them leave a Gaussian tail of 2e-9 per element.
The deterministic worst case (n u times the sum of |x w|, carried through |W|) is elementwise too, but with these weights it
exceeds o2 itself 400-fold and the logit 10^7-fold: no gate at all.  Nothing here is fitted to GPU results: the tests print the
worst err / B per stage so that the headroom is visible.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

U32 = 2.0 ** -24
SAFETY = 6.0
U_PROD = {"f32": U32, "f16x3": 5 * 2.0 ** -22, "bf16x3": 2.0 ** -20}
# the arithmetic of each stage (c_conv1, c_conv2, c_conv3, Dense) per head mode (include/ovn_hip.h: ovn_set_head_precision):
#   f32     c_conv1 + c_conv2 on the fp32 matrix cores (|l - r| formed exactly, delta_head.hip), c_conv3 + Dense fp32
#   f16x3   c_conv1 / c_conv2 split on the fp16 matrix cores (min form), c_conv3 + Dense fused and split (c3_dense.hip)
#   bf16x3  c_conv1 / c_conv2 split on the bf16 matrix cores (min form), c_conv3 + Dense fp32
#   generic any conv1NetworkHead_conv1size but 15: fp32 FMAs on |l - r| (delta_head_generic.hip), fp32 after it
HEAD_STAGE_MODE = {"f32": ("f32", "f32", "f32", "f32"), "f16x3": ("f16x3", "f16x3", "f16x3", "f16x3"),
                   "bf16x3": ("bf16x3", "bf16x3", "f32", "f32"), "generic": ("f32", "f32", "f32", "f32")}
U_SUB = 2.0 ** -150        # half the spacing of fp32 subnormals: the absolute rounding floor of any fp32 result
HEAD_FORM = {"f32": "abs", "f16x3": "min", "bf16x3": "min", "generic": "abs"}


def ratio(gpu, ref, bound) -> float:
    """Worst |gpu - ref| / bound over the tensor (<= 1 passes).  An element whose bound is 0 must match exactly; NaN fails."""
    err = np.abs(np.asarray(gpu, np.float64) - np.asarray(ref, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    return float(np.max(r)) if r.size else 0.0


# --------------------------------------------------------------------------------------------------------------------------------
# Delta head, one pair, fp64: values and magnitudes of every stage
# --------------------------------------------------------------------------------------------------------------------------------

def _w(weights, name):
    return np.asarray(weights[name], np.float64)


def min_form_parts(l: np.ndarray, r: np.ndarray, weights, s: int = 15):
    """The three terms of c_conv1 in min form, fp64: (lin_l (W, G, 64), lin_r (G, 64), M (W, G, 64), c) with
    o1 = b1 + lin_l + lin_r - 2 M.  lin_l[i, jb] = sum_{dj,c} l'[i, c] W1[dj, c], lin_r[jb] = sum_{dj,c} r'[s jb + dj, c] W1[dj, c],
    M[i, jb] = sum_{dj,c} min(l'[i, c], r'[s jb + dj, c]) W1[dj, c].  W = l.shape[0], G = W // s."""
    l = np.asarray(l, np.float64)
    r = np.asarray(r, np.float64)
    wd = l.shape[0]
    g = wd // s
    c = -min(0.0, float(l.min()), float(r.min()))
    lp, rp = l + c, r + c
    w1 = _w(weights, "c_conv1/kernel").reshape(s, 128, 64)
    lin_l = np.repeat((lp @ w1.sum(axis=0))[:, None, :], g, axis=1)
    lin_r = rp[:g * s].reshape(g, s * 128) @ w1.reshape(s * 128, 64)
    mn = np.minimum(lp[:, None, :], rp[None, :g * s, :])                      # (W, g s, 128)
    M = mn.reshape(wd * g, s * 128) @ w1.reshape(s * 128, 64)
    return lin_l, lin_r, M.reshape(wd, g, 64), c


def _c1(x_ij, w1, s, width=None):
    """sum_{dj,c} x[i, s jb + dj, c] w1[dj, c, o] for x (n, >= G s, 128); G = width // s, width = n by default (the volume's W)."""
    n = x_ij.shape[0]
    g = (width or n) // s
    return (x_ij[:, :g * s].reshape(n * g, s * 128) @ w1.reshape(s * 128, 64)).reshape(n, g, 64)


def _c1_abs_rows(l64, r64, w1, s, rows=32):
    """c_conv1 on |l - r| without its bias and the root-sum-square of its terms, (W, G, 64) each, `rows` rows of l at a time: the
    abs form of `head_pair` at a width other than 360, whose (W, W, 128) intermediates would take ~270 MB each at W = 512."""
    wd = l64.shape[0]
    g = wd // s
    w1sq = np.square(w1)
    val, var = np.empty((wd, g, 64)), np.empty((wd, g, 64))
    for i0 in range(0, wd, rows):
        d = np.abs(l64[i0:i0 + rows, None, :] - r64[None, :g * s, :])
        val[i0:i0 + rows] = _c1(d, w1, s, wd)
        var[i0:i0 + rows] = _c1(np.square(d), w1sq, s, wd)
    return val, np.sqrt(var)


def head_tail(o1: np.ndarray, weights, s: int = 15, wf=None, relu: bool = True):
    """c_conv2 (+ ReLU), c_conv3 (+ ReLU), Dense on a c_conv1 output (W, G, 64).  `wf`: applied to every weight and bias first
    (np.abs: the magnitude chain; np.square: the variance chain), relu=False for those.  Returns (o2 (G, G, 128), o3 (G-2, G-2, 256),
    logit)."""
    f = wf or (lambda a: a)
    g = o1.shape[1]
    o2 = _conv2(o1, f(_w(weights, "c_conv2/kernel")), f(_w(weights, "c_conv2/bias")), s)
    if relu:
        o2 = np.maximum(o2, 0)
    o3 = _conv3(o2, f(_w(weights, "c_conv3/kernel")), f(_w(weights, "c_conv3/bias")))
    if relu:
        o3 = np.maximum(o3, 0)
    logit = float(o3.reshape(-1) @ f(_w(weights, "overlap_output/kernel")).reshape(-1) + f(_w(weights, "overlap_output/bias")).sum())
    return o2, o3, logit


def _conv2(o1, w2, b2, s):
    g = o1.shape[1]
    x = o1[:g * s].reshape(g, s, g, 64).transpose(0, 2, 1, 3).reshape(g * g, s * 64)
    return (x @ w2.reshape(s * 64, 128) + b2).reshape(g, g, 128)


def _conv3(o2, w3, b3):
    g = o2.shape[0]
    o3 = np.zeros((g - 2, g - 2, 256))
    for dy in range(3):
        for dx in range(3):
            o3 += o2[dy:dy + g - 2, dx:dx + g - 2] @ w3[dy, dx]
    return o3 + b3


def head_pair(l: np.ndarray, r: np.ndarray, weights, s: int = 15, o1: Optional[np.ndarray] = None) -> dict:
    """fp64 values of every Delta-head stage of the pair (l, r), each (W, 128), plus what `head_bounds` needs: the sizes of the
    c_conv1 terms in both forms.  `o1`: a (possibly perturbed) c_conv1 output to push through the rest instead of the exact one
    (the fault models of the tests).  At W != 360 every head mode runs the exact fp32 kernels (|l - r| formed exactly): only the
    abs form is kept, computed a few rows at a time."""
    l64 = np.asarray(l, np.float64)
    r64 = np.asarray(r, np.float64)
    w1 = _w(weights, "c_conv1/kernel").reshape(s, 128, 64)
    b1 = _w(weights, "c_conv1/bias")
    if l64.shape[0] != 360:
        c1v, rms_abs = _c1_abs_rows(l64, r64, w1, s)
        o1x = b1 + c1v
        if o1 is None:
            o1 = o1x
        o2, o3, logit = head_tail(o1, weights, s)
        overlap = 1.0 / (1.0 + math.exp(-logit)) if logit > -700 else 0.0
        c = -min(0.0, float(l64.min()), float(r64.min()))
        span = float(max(l64.max() + c, r64.max() + c, 0.0))
        return {"o1": o1, "o2": o2, "o3": o3, "logit": logit, "overlap": overlap, "s": s, "span": span,
                "c1": {"abs": (np.abs(b1) + np.abs(c1v), rms_abs)}}
    diff = np.abs(l64[:, None, :] - r64[None, :, :])
    o1x = b1 + _c1(diff, w1, s)
    if o1 is None:
        o1 = o1x
    o2, o3, logit = head_tail(o1, weights, s)
    w1sq = np.square(w1)
    lin_l, lin_r, M, c = min_form_parts(l64, r64, weights, s)
    lp, rp = l64 + c, r64 + c
    mn = np.minimum(lp[:, None, :], rp[None, :, :])
    rms_min = np.sqrt(_c1(lp[:, None, :] ** 2 + rp[None, :, :] ** 2 + 4 * mn ** 2, w1sq, s))
    val_min = np.abs(b1) + np.abs(lin_l) + np.abs(lin_r)[None] + 2 * np.abs(M)
    rms_abs = np.sqrt(_c1(diff ** 2, w1sq, s))
    val_abs = np.abs(b1) + np.abs(o1x - b1)
    overlap = 1.0 / (1.0 + math.exp(-logit)) if logit > -700 else 0.0
    return {"o1": o1, "o2": o2, "o3": o3, "logit": logit, "overlap": overlap, "s": s, "span": float(max(lp.max(), rp.max(), 0.0)),
            "c1": {"min": (val_min, rms_min), "abs": (val_abs, rms_abs)}}


def pow2_scale(m: float, clamp: bool = True) -> float:
    """ovn_pow2_scale_for (csrc/ovn_internal.h): 2^(14 - e) with 2^(e-1) <= m < 2^e, clamped at 2^+-100; 1 for m = 0."""
    if not (m > 0 and m < 3.0e38):
        return 1.0
    k = 14 - math.frexp(m)[1]
    return 2.0 ** (min(100, max(-100, k)) if clamp else k)


def _floor(mode: str, xmax: float, wabs_sum):
    """Absolute error floor of a stage whose operands are scaled by pow2_scale(xmax) (f16x3 only; module doc): 2^-25 / scale per
    operand, x 2 for the weights' own floor, x 2 for the hi and lo terms."""
    return 4 * 2.0 ** -25 / pow2_scale(xmax) * wabs_sum if mode == "f16x3" else 0.0


def _sigma(mode: str, n: int, val, rms):
    """Size of the own rounding error of one contraction of n products whose value has size `val` and whose terms have
    root-sum-square `rms` (module doc): u_prod rms + sqrt(n) u (|val| + rms)."""
    return U_PROD[mode] * rms + math.sqrt(n) * U32 * (np.abs(val) + rms)


def head_bounds(h: dict, weights, mode: str) -> dict:
    """Elementwise error bounds of o1, o2, o3, the logit and the overlap of a `head_pair` result in head mode `mode`
    ('f32', 'f16x3', 'bf16x3' or 'generic'): B_k = SAFETY sigma_k, sigma_k^2 = own_k^2 + conv(W_k^2, sigma_{k-1}^2)."""
    s = h["s"]
    m1, m2, m3, ml = HEAD_STAGE_MODE[mode]
    sq = np.square
    w2, w3 = _w(weights, "c_conv2/kernel"), _w(weights, "c_conv3/kernel")
    wd = _w(weights, "overlap_output/kernel").reshape(-1)
    if HEAD_FORM[mode] not in h["c1"]:
        raise ValueError("head mode %s at a feature width other than 360: every head mode runs the fp32 kernels there ('f32')" % mode)
    val1, rms1 = h["c1"][HEAD_FORM[mode]]
    a1 = np.abs(_w(weights, "c_conv1/kernel")).reshape(-1, 64).sum(axis=0)
    a2 = np.abs(w2).reshape(-1, 128).sum(axis=0)
    a3 = np.abs(w3).reshape(-1, 256).sum(axis=0)
    # largest operand of each stage as the kernels scale it: 4 span (l', r' and 2 min), the bound 4 span max sum|W1| + |b1| of
    # c_conv1's output (delta_prepare_split_kernel: s1r, sT), the pair's largest o2 (c3_dense.hip)
    x1, x2 = 4 * h["span"], 4 * h["span"] * float(a1.max()) + float(np.abs(_w(weights, "c_conv1/bias")).max())
    s1 = _sigma(m1, s * 128, val1, rms1) + _floor(m1, x1, a1)
    pre2 = _conv2(h["o1"], w2, _w(weights, "c_conv2/bias"), s)
    s2 = np.sqrt(sq(_sigma(m2, s * 64, pre2, np.sqrt(_conv2(sq(h["o1"]), sq(w2), 0.0, s))) + _floor(m2, x2, a2))
                 + _conv2(sq(s1), sq(w2), 0.0, s))
    pre3 = _conv3(h["o2"], w3, _w(weights, "c_conv3/bias"))
    s3 = np.sqrt(sq(_sigma(m3, 9 * 128, pre3, np.sqrt(_conv3(sq(h["o2"]), sq(w3), 0.0))) + _floor(m3, float(h["o2"].max()), a3))
                 + _conv3(sq(s2), sq(w3), 0.0))
    o3 = h["o3"].reshape(-1)
    sl = math.sqrt(float(_sigma(ml, o3.size, h["logit"], math.sqrt(float(sq(o3) @ sq(wd))))) ** 2 + float(sq(s3).reshape(-1) @ sq(wd)))
    bl = SAFETY * sl
    return {"o1": SAFETY * s1, "o2": SAFETY * s2, "o3": SAFETY * s3, "logit": bl, "overlap": overlap_bound(h["logit"], bl)}


def corr_pair(l: np.ndarray, r: np.ndarray) -> dict:
    """Correlation vector of the pair (W,), W = l.shape[0], with its elementwise bounds in both forms:
        corr[k] = sum_j sum_c l[(k + j + W // 2) mod W, c] r[j, c]
      direct    one fp32 contraction of W x 128 products (corr_head.hip): SAFETY (u rms + sqrt(n) u (|v| + rms))
                per shift, plus the subnormal floor of n fp32 products.
      spectral  corr_spectral.hip: each spectrum X^[f, c] = sum_i x[i, c] e^(-2 pi i f i / 360) is a 360-term contraction split on
                the fp16 matrix cores, its operands scaled by 2^k from the scan's largest |value| (unclamped: dft_f16x3_kernel);
                the spectral product C^[f] = sum_c L^ conj(R^) is summed over 128 channels in fp32; the inverse transform is
                fp64.  Errors are carried as in the head (independent errors add in quadrature): per coefficient
                    sigma_X[f, c] = u_prod ||x_c||_2 + sqrt(360) u (|X^| + ||x_c||_2) + sqrt(360) 4 2^-25 / scale + U_SUB
                    sigma_C[f]^2  = sum_c (|R^|^2 sigma_L^2 + |L^|^2 sigma_R^2) + (sqrt(128) u (|C^| + rms_C))^2
                and the inverse transform (1 / 360) sum_f C^[f] e^(...) carries sqrt(2 sum_f sigma_C^2) / 360 to every shift (f and
                360 - f are conjugates: their errors add coherently).  360 columns only (the spectral route refuses other widths):
                at W != 360 the result has no 'spectral' entry."""
    l64 = np.asarray(l, np.float64)
    r64 = np.asarray(r, np.float64)
    wd = l64.shape[0]
    jj = np.arange(wd)
    idx = (np.arange(wd)[:, None] + jj[None, :] + wd // 2) % wd
    corr = (l64 @ r64.T)[idx, jj[None, :]].sum(axis=1)
    rms = np.sqrt((np.square(l64) @ np.square(r64).T)[idx, jj[None, :]].sum(axis=1))
    n = wd * 128
    direct = SAFETY * _sigma("f32", n, corr, rms) + n * U_SUB + U_SUB
    if wd != 360:
        return {"corr": corr, "direct": direct}
    L, R = np.fft.fft(l64, axis=0), np.fft.fft(r64, axis=0)                  # (360 f, 128 c)

    def sig_x(X, x):
        nrm = np.sqrt(np.square(x).sum(axis=0))[None, :]
        fl = math.sqrt(360) * 4 * 2.0 ** -25 / pow2_scale(float(np.abs(x).max()), clamp=False)
        return U_PROD["f16x3"] * nrm + math.sqrt(360) * U32 * (np.abs(X) + nrm) + fl + U_SUB
    sl, sr = sig_x(L, l64), sig_x(R, r64)
    P = L * np.conj(R)
    C = P.sum(axis=1)
    rms_c = np.sqrt(np.square(np.abs(P)).sum(axis=1))
    var_c = (np.square(np.abs(R)) * sl ** 2 + np.square(np.abs(L)) * sr ** 2).sum(axis=1) \
        + np.square(math.sqrt(128) * U32 * (np.abs(C) + rms_c) + U_SUB)
    spectral = SAFETY * math.sqrt(2 * float(var_c.sum())) / 360 + U32 * np.abs(corr) + U_SUB
    return {"corr": corr, "direct": direct, "spectral": spectral}


def overlap_bound(logit: float, dlogit: float) -> float:
    """|d overlap| allowed by a logit error bound dlogit: the sigmoid's slope is at most max over [logit +- dlogit] of s (1 - s)."""
    lo, hi = logit - dlogit, logit + dlogit
    z = 0.0 if lo <= 0 <= hi else min(abs(lo), abs(hi))
    sg = 1.0 / (1.0 + math.exp(-z)) if z < 700 else 1.0
    return sg * (1 - sg) * dlogit + 2 * U32


# --------------------------------------------------------------------------------------------------------------------------------
# Leg
# --------------------------------------------------------------------------------------------------------------------------------

def _leg_convs(x, k, b, stride):
    """fp64 pre-activation of one leg layer on x (n, h, w, c) and the root-sum-square of its terms."""
    import torch
    from oracle import overlapnet_oracle as O
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)
    back = lambda y: y.permute(0, 2, 3, 1).numpy()
    pre = back(O._conv_valid(t(x), k, b, stride, False, torch.float64))
    rms = np.sqrt(back(O._conv_valid(t(np.square(x)), np.square(k), np.zeros_like(b), stride, False, torch.float64)))
    return pre, rms


def leg_layer_bound(x, kernel, bias, stride, modes=("f16x3", "f32")):
    """One leg layer in isolation on its exact fp32 input x (n, h, w, c): (fp64 output after ReLU, {mode: elementwise bound})."""
    k, b = np.asarray(kernel, np.float64), np.asarray(bias, np.float64)
    pre, rms = _leg_convs(np.asarray(x, np.float64), k, b, stride)
    n = k.shape[0] * k.shape[1] * k.shape[2]
    return np.maximum(pre, 0), {m: SAFETY * _sigma(m, n, pre, rms) for m in modes}


def leg_with_bounds(images_nhwc: np.ndarray, weights, modes=("f16x3", "f32"), model_cfg=None) -> dict:
    """The fp64 leg computed ONCE, with the elementwise bound of every layer output in each of `modes` ('f32', 'f16x3':
    ovn_set_leg_precision): {mode: [(layer name, fp64 output (n, h, w, c), bound)]}.  As in the head, a layer's own error
    (u_prod rms + sqrt(n) u (|v| + rms)) and the carried error of its input (conv(W^2, sigma^2)) add in quadrature."""
    import torch
    from oracle import overlapnet_oracle as O
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).permute(0, 3, 1, 2)
    back = lambda y: y.permute(0, 2, 3, 1).numpy()
    out = {m: [] for m in modes}
    sig = {m: None for m in modes}
    x = np.asarray(images_nhwc, np.float64)
    for name, stride in O._leg_plan(model_cfg):
        k = np.asarray(weights[name + "/kernel"], np.float64)
        b = np.asarray(weights[name + "/bias"], np.float64)
        n = k.shape[0] * k.shape[1] * k.shape[2]
        pre, rms = _leg_convs(x, k, b, stride)
        x = np.maximum(pre, 0)
        for m in modes:
            var = np.square(_sigma(m, n, pre, rms))
            if sig[m] is not None:
                var = var + back(O._conv_valid(t(np.square(sig[m])), np.square(k), np.zeros_like(b), stride, False, torch.float64))
            sig[m] = np.sqrt(var)
            out[m].append((name, x, SAFETY * sig[m]))
    return out


# --------------------------------------------------------------------------------------------------------------------------------
# Feature volumes on the value edges of the Delta head's fast paths (shared by the CPU fault-power test and the GPU tests)
# --------------------------------------------------------------------------------------------------------------------------------

def _relu_vol(rng, k=1, mean=0.2, width=360):
    return np.maximum(rng.normal(mean, 1.0, size=(k, width, 128)), 0).astype(np.float32)


def value_edge_sets(seed: int = 0, width: int = 360) -> Dict[str, np.ndarray]:
    """name -> (k, width, 128) float32 volumes.  Volume 0 is the query of the 1-vs-N routes, all of them its candidates (the
    single_column and pow2_edge sets are also swept with other queries: their edges are properties of the query)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    out = {}
    # -0.0: scattered through query and candidates, an all -0.0 volume, -0.0 as a volume's minimum (no negative value anywhere)
    v = _relu_vol(rng, 4, width=width)
    for i in (0, 1):
        z = v[i] == 0
        v[i][z & (rng.random(z.shape) < 0.5)] = f32(-0.0)
    v[2] = f32(-0.0)
    v[3][v[3] == 0] = f32(-0.0)
    out["neg_zero"] = v
    # subnormals: a volume of subnormals only, subnormals in place of the zeros of O(1) volumes
    v = _relu_vol(rng, 4, width=width)
    v[1] = (rng.random((width, 128)) * 1e-39).astype(f32)
    for i in (0, 2):
        z = v[i] == 0
        v[i][z] = (rng.random(int(z.sum())) * 1e-38).astype(f32)
    out["subnormal"] = v
    # one value of -1e-30 in the query (shift on, no compaction), and in a candidate
    v = _relu_vol(rng, 3, width=width)
    v[0][:, 100:] = 0
    v[0, 17, 5] = f32(-1e-30)
    v[2, 200 * width // 360, 60] = f32(-1e-30)
    out["tiny_negative"] = v
    # largest values at exactly 2^k and one ulp around it: volumes 0, 1, 2 (4, 4 - ulp, 4 + ulp) each serve as the query of a
    # sweep over all six (tests/test_gpu_error_bounds.py), so the query's own bucket and the candidates' buckets meet in both
    # orders: both sides of the cache-row validity rule and of the scale bucket edge
    base = _relu_vol(rng, 6, width=width)
    tops = [f32(4.0), np.nextafter(f32(4.0), f32(0)), np.nextafter(f32(4.0), f32(8)), f32(4.0), np.nextafter(f32(4.0), f32(8)),
            np.nextafter(f32(4.0), f32(0))]
    for i, t in enumerate(tops):
        base[i] = np.minimum(base[i], f32(3.5))
        base[i, 11 + i, 7 * i] = t
    out["pow2_edge"] = base
    # channels alive in exactly one query column (O(1) value), live counts 97, 111, 112, 113 -> packed last slices of 1, 15, 16, 17
    q = np.zeros((5, width, 128), f32)
    perm = rng.permutation(128)
    for i, live in enumerate((97, 111, 112, 113)):
        ch = perm[:live]
        q[i][:, ch] = np.maximum(rng.normal(0.2, 1.0, size=(width, live)), 0)
        q[i][:, ch[:8]] = 0
        q[i][rng.integers(0, width, 8), ch[:8]] = f32(1.0)          # alive in one column each
    q[4] = _relu_vol(rng, width=width)[0]
    out["single_column"] = q
    # exact ties: duplicated columns, and the query among its own candidates
    v = _relu_vol(rng, 3, width=width)
    v[0][width - width // 2:] = v[0][:width // 2]
    v[1] = v[0]
    v[2][:, :64] = v[0][:, :64]
    out["ties"] = v
    # wide ranges in one volume, and large spans
    v = _relu_vol(rng, 4, width=width)
    v[0] *= np.where(rng.random((width, 128)) < 0.5, f32(1e-6), f32(1e4)).astype(f32)
    v[2] *= f32(1e20)
    v[3] *= f32(1e30)
    v[3][:, 64:] = 0
    v[3][10:] = 0                # (the correlation sums of 1e30 x 1e4 must stay inside fp32)
    out["wide_range"] = v
    return out
