"""TEST INFRASTRUCTURE: the f16x3 error bound of the Delta head at feature widths other than 360.

`oracle/error_bounds.py` keeps the min-form entry of c_conv1 (`h["c1"]["min"]`) only at W = 360, because off 360 every head mode
ran the fp32 kernels; `head_bounds(h, w, "f16x3")` raises there for that reason alone.  With the split width route
(csrc/delta_head_w_f16x3.hip, `ovn_set_head_width_split`) the f16x3 arithmetic exists at every width, and this helper adds the
missing entry from the module's own parts, a few rows of l at a time like `_c1_abs_rows`:

    val = |b1| + |lin_l| + |lin_r| + 2 |M|                          (E.min_form_parts)
    rms = sqrt(c1(l'^2 + r'^2 + 4 min(l', r')^2, W1^2))              l' = l + c, r' = r + c, c = -min(0, smallest value of the pair)

after which the unchanged `E.head_bounds(h, w, "f16x3")` returns B = 6 sigma for o1, o2, o3, the logit and the overlap.  Nothing is
fitted.  What the bound assumes and what the kernels do:
  * Form.  The kernels take the ABS form (|l - r| in fp32, then scaled and split); the min form's three cancelling terms make its
    val and rms the larger ones (l'^2 + r'^2 + 4 min^2 >= (l - r)^2, |lin_l| + |lin_r| + 2 |M| >= |c1(|l - r|)|), so the bound
    covers the abs form with room to spare.
  * Floor.  `head_bounds` prices the fp16 subnormal floor with the operand scales pow2_scale(4 span) for c_conv1 and
    pow2_scale(4 span max sum|W1| + |b1|max) for c_conv2.  The kernels scale by ovn_pow2_scale_for(span) and
    ovn_pow2_scale_for(|b1|max + span max sum|W1|): both arguments are smaller, the scales at least as large, the floor at most the
    one priced.
  * c_conv3 and Dense run in fp32 on this route; the bound prices them as split stages, whose error is the larger one."""
import numpy as np

from oracle import error_bounds as E


def min_entry(l, r, weights, s=15, rows=32):
    """(val, rms) of c_conv1 in min form, (W, G, 64) each, at any width."""
    l64, r64 = np.asarray(l, np.float64), np.asarray(r, np.float64)
    wd = l64.shape[0]
    g = wd // s
    w1 = E._w(weights, "c_conv1/kernel").reshape(s, 128, 64)
    b1 = E._w(weights, "c_conv1/bias")
    lin_l, lin_r, M, c = E.min_form_parts(l64, r64, weights, s)
    val = np.abs(b1) + np.abs(lin_l) + np.abs(lin_r)[None] + 2 * np.abs(M)
    lp, rp = l64 + c, r64 + c
    w1sq = np.square(w1)
    var = np.empty((wd, g, 64))
    for i0 in range(0, wd, rows):
        a = lp[i0:i0 + rows, None, :]
        b = rp[None, :g * s, :]
        var[i0:i0 + rows] = E._c1(np.square(a) + np.square(b) + 4 * np.square(np.minimum(a, b)), w1sq, s, wd)
    return val, np.sqrt(var)


def head_pair_split(l, r, weights, s=15, o1=None):
    """E.head_pair with the min-form entry present at every width."""
    h = E.head_pair(l, r, weights, s, o1=o1)
    if "min" not in h["c1"]:
        h["c1"]["min"] = min_entry(l, r, weights, s)
    return h


def bounds(h, weights):
    """The elementwise f16x3 bounds of a `head_pair_split` result."""
    return E.head_bounds(h, weights, "f16x3")
