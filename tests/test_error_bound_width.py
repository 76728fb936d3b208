"""CPU: the elementwise error bounds at feature widths other than 360 (the fp32 heads at a runtime width, delta_head.hip and corr_head.hip).

The fp64 restatement (oracle/error_bounds.py, tests/_corr_norm_ref.py) is pinned to the oracle at widths that sit on the edges of the
width kernels' tiling, and every fault below -- built as the output a faulty width kernel would produce and pushed through the rest
of its head -- must be rejected by the bound of the fp32 arithmetic those kernels run in every head mode.  The test prints which of
the faults the fixed tolerances of tests/test_gpu_feature_width.py (overlap 1e-4, logit 1e-3 (1 + |logit|), corr 2e-5 max|corr|)
would have accepted."""
import numpy as np
import pytest

from oracle import overlapnet_oracle as O
from oracle import error_bounds as E
from tests import _corr_norm_ref as R
from tools import synthetic as S

NORM_BLK = 24                  # columns per block of the normalisation statistics (csrc/ovn_internal.h: OVN_NORM_BLK)
_WEIGHTS = {}


def _weights(fw, seed=0):
    if (fw, seed) not in _WEIGHTS:
        _WEIGHTS[(fw, seed)] = S.make_test_weights(4, seed=seed, feat_w=fw)
    return _WEIGHTS[(fw, seed)]


def _relu(fw, k, seed):
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, fw, 128)), 0).astype(np.float32)
    for i in range(k):
        v[i][:, rng.permutation(128)[:32]] = 0
    return v


@pytest.mark.parametrize("fw", [45, 59, 385, 512])
def test_restatement_matches_the_oracle_at_other_widths(fw):
    """head_pair / corr_pair / corr_norm_pair / known_bin at W = 45 (G = 3), 59 (14 unread columns), 385 (a one-column last Gram
    panel), 512 (G = 34) against the oracle's heads."""
    w = _weights(fw, seed=3)
    sets = E.value_edge_sets(seed=1, width=fw)
    for name, i, j in (("neg_zero", 1, 0), ("tiny_negative", 2, 0), ("wide_range", 0, 1)):
        l, r = sets[name][i], sets[name][j]
        assert l.shape == (fw, 128)
        h = E.head_pair(l, r, w)
        _, lg, it = O.delta_head_forward(l[None, None], r[None, None], w, return_intermediates=True)
        assert h["o2"].shape == (fw // 15, fw // 15, 128) and h["o3"].shape == (fw // 15 - 2, fw // 15 - 2, 256)
        for k in ("o1", "o2", "o3"):
            assert np.max(np.abs(h[k] - it[k])) <= 1e-12 * (np.max(np.abs(it[k])) + 1e-300), (name, k)
        assert abs(h["logit"] - lg[0]) <= 1e-12 * (1 + abs(lg[0]))
        B = E.head_bounds(h, w, "f32")
        assert all(np.all(np.asarray(B[k]) > 0) for k in ("o2", "o3", "logit"))
        with pytest.raises(ValueError):            # no min form off 360: the width kernels are fp32 in every head mode
            E.head_bounds(h, w, "f16x3")
        corr = O.correlation_head_forward(l[None, None], r[None, None])[0]
        c = E.corr_pair(l, r)
        assert set(c) == {"corr", "direct"}
        assert np.max(np.abs(c["corr"] - corr)) <= 1e-12 * np.max(np.abs(corr))
    v = R.edge_volume(5, fw)
    assert v.shape == (fw, 128)
    r = R.rolled(v, 7)
    for mode in R.MODES:
        ln, rn = R.normalize64(v, mode), R.normalize64(r, mode)
        corr = O.correlation_head_forward(ln[None, None], rn[None, None])[0]
        c = R.corr_norm_pair(v, r, mode)
        assert np.max(np.abs(c["corr"] - corr)) <= 1e-12 * np.max(np.abs(corr)), mode
        assert set(c) == {"corr", "direct"} and np.all(c["direct"] > 0)
        # the literal RangePadding2D (padding W // 2) + sliding-window form: the wrap at odd W from the layer's own definition
        lit = O.correlation_literal(ln[None, None], rn[None, None])[0, 0, :, 0]
        assert np.max(np.abs(c["corr"] - lit)) <= 1e-12 * np.max(np.abs(lit)), mode
        if mode == "euclidean":
            lit = O.correlation_literal(v[None, None], r[None, None], "euclidean")[0, 0, :, 0]
            assert np.max(np.abs(c["corr"] - lit)) <= 1e-12 * np.max(np.abs(lit))
    x = _relu(fw, 1, fw)[0]
    for s in (0, 1, fw // 2, fw - 1, 7):
        corr = O.correlation_head_forward(x[None, None], R.rolled(x, s)[None, None])[0]
        assert int(np.argmax(corr)) == R.known_bin(s, fw), (fw, s)


def test_360_defaults_are_the_360_forms():
    """The width arguments default to 360 and the odd-width wrap reduces to the 360 one there."""
    assert [R.known_bin(s) for s in (0, 1, 180, 359)] == [180, 179, 0, 181]
    assert [R.known_bin(s, 360) for s in (0, 1, 180, 359)] == [180, 179, 0, 181]
    a, b = E.value_edge_sets(), E.value_edge_sets(width=360)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(R.edge_volume(2), R.edge_volume(2, 360))
    assert "spectral" in E.corr_pair(a["neg_zero"][0], a["neg_zero"][1])


# ---- fault power at other widths ------------------------------------------------------------------------------------------------

def _tail_from_o2(o2, w):
    """c_conv3 (+ ReLU) and the Dense layer on a c_conv2 output (G, G, 128), fp64."""
    o3 = np.maximum(E._conv3(o2, E._w(w, "c_conv3/kernel"), E._w(w, "c_conv3/bias")), 0)
    logit = float(o3.reshape(-1) @ E._w(w, "overlap_output/kernel").reshape(-1) + E._w(w, "overlap_output/bias").sum())
    return {"o2": o2, "o3": o3, "logit": logit, "overlap": 1.0 / (1.0 + np.exp(-logit))}


def _fault_gemm2_last_row_tile(l, r, w):
    """delta_c12_kernel run with MT = G // 16 row tiles instead of ceil(G / 16): the o2 rows of the last tile are never written
    (left at zero here)."""
    h = E.head_pair(l, r, w)
    o2 = h["o2"].copy()
    g = o2.shape[0]
    o2[16 * (g // 16):] = 0
    return h, _tail_from_o2(o2, w)


def _fault_conv1_reads_late(l, r, w):
    """c_conv1 reads r one column late (s jb + dj + 1): the last tap of the last group reads the first unread tail column."""
    fw = l.shape[0]
    g = fw // 15
    cols = np.arange(15 * g) + 1
    assert cols.max() < fw
    d = np.abs(l.astype(np.float64)[:, None, :] - r.astype(np.float64)[None, cols, :])
    o1 = E._w(w, "c_conv1/bias") + E._c1(d, E._w(w, "c_conv1/kernel").reshape(15, 128, 64), 15)
    return E.head_pair(l, r, w), E.head_pair(l, r, w, o1=o1)


def _corr_rolled_wrap(l, r):
    """corr_head_kernel wrapping with (W + 1) // 2 instead of W // 2: at odd W every bin reads its right-hand neighbour."""
    c = E.corr_pair(l, r)
    fw = l.shape[0]
    assert fw % 2 == 1
    jj = np.arange(fw)
    idx = (np.arange(fw)[:, None] + jj[None, :] + (fw + 1) // 2) % fw
    bad = (l.astype(np.float64) @ r.astype(np.float64).T)[idx, jj[None, :]].sum(axis=1)
    return c, bad


def _corr_last_panel_dropped(l, r):
    """The Gram matrix's last 16-column panel (partial at W % 16 != 0) never folded into the correlation."""
    c = E.corr_pair(l, r)
    fw = l.shape[0]
    keep = 16 * ((fw - 1) // 16)
    r2 = r.astype(np.float64).copy()
    r2[keep:] = 0
    return c, E.corr_pair(l, r2)["corr"]


def _affine_without_last_block(v, mode):
    """(m, a, s) of ovn_corr_norm_affine with its last (partial) 24-column block lost from the statistics; the mean still divides by
    W, as the kernel does."""
    x = np.asarray(v, np.float64)
    fw = x.shape[0]
    nb = -(-fw // NORM_BLK)
    xs = x[:NORM_BLK * (nb - 1)]
    if mode == "scaling":
        lo, hi = xs.min(axis=0, keepdims=True), xs.max(axis=0, keepdims=True)
        return lo, 0.0, 1.0 / ((hi - lo) + 1e-6)
    m, a = (xs.sum(axis=0, keepdims=True) / fw, 1e-5) if mode == "standardization" else (np.zeros((1, 128)), 0.0)
    q = np.square((xs - m) + a).sum(axis=0, keepdims=True)
    return m, a, 1.0 / np.sqrt(np.maximum(q, 1e-12))


def _corr_norm_last_block_dropped(l, r, mode):
    ref = R.corr_norm_pair(l, r, mode)
    ln, rn = [((np.asarray(x, np.float64) - m) + a) * s for x, (m, a, s) in ((l, _affine_without_last_block(l, mode)),
                                                                             (r, _affine_without_last_block(r, mode)))]
    return ref, E.corr_pair(ln, rn)["corr"]


def _old_head(ref, bad):
    return abs(bad["overlap"] - ref["overlap"]) <= 1e-4 and abs(bad["logit"] - ref["logit"]) <= 1e-3 * (1 + abs(ref["logit"]))


def _old_corr(ref, bad):
    return np.max(np.abs(bad - ref)) <= 2e-5 * np.max(np.abs(ref))


def _edge_norm_volume(seed, fw):
    """edge_volume with channel 20 at its largest value in the last column and channel 21 at its smallest, so that the last
    block of the normalisation statistics decides a minimum and a maximum."""
    v = R.edge_volume(seed, fw)
    v[fw - 1, 20] = np.float32(9.0)
    v[fw - 1, 21] = np.float32(-9.0)
    return v


def _width_faults():
    out = []
    for fw in (512, 255):                           # G = 34: MT 3 -> 2;  G = 17: MT 2 -> 1
        w = _weights(fw)
        v = _relu(fw, 2, fw)
        ref, bad = _fault_gemm2_last_row_tile(v[0], v[1], w)
        out.append(("head", "gemm2_last_row_tile_lost W=%d G=%d" % (fw, fw // 15), ref, bad, ("o2", "o3", "logit", "overlap"), w))
    w = _weights(59)
    v = _relu(59, 2, 59)
    ref, bad = _fault_conv1_reads_late(v[0], v[1], w)
    out.append(("head", "c_conv1_reads_r_one_column_late W=59", ref, bad, ("o2", "o3", "logit", "overlap"), w))
    for fw in (45, 59, 255, 375, 385, 495):
        v = _relu(fw, 2, fw + 1)
        c, bad = _corr_rolled_wrap(v[0], v[1])
        out.append(("corr", "corr_wrap_(W+1)//2 W=%d" % fw, c["corr"], bad, c["direct"], None))
    for fw in (45, 385, 497):
        v = _relu(fw, 2, fw + 2)
        c, bad = _corr_last_panel_dropped(v[0], v[1])
        out.append(("corr", "last_gram_panel_dropped W=%d (%d columns)" % (fw, fw - 16 * ((fw - 1) // 16)), c["corr"], bad,
                    c["direct"], None))
    for fw in (45, 385):
        l, r = _edge_norm_volume(1, fw), _edge_norm_volume(2, fw)
        for mode in ("euclidean", "scaling", "standardization"):
            c, bad = _corr_norm_last_block_dropped(l, r, mode)
            out.append(("corr", "norm_stats_last_block_dropped %s W=%d" % (mode, fw), c["corr"], bad, c["direct"], None))
    return out


def test_bound_rejects_every_width_fault():
    old_accepts = []
    faults = _width_faults()
    for kind, name, ref, bad, bound, w in faults:
        if kind == "head":
            B = E.head_bounds(ref, w, "f32")
            worst = {k: E.ratio(bad[k], ref[k], B[k]) for k in bound}
            old = _old_head(ref, bad)
            assert np.max(np.abs(bad["o2"] - ref["o2"])) > 0, name
        else:
            worst = {"corr": E.ratio(bad, ref, bound)}
            old = _old_corr(ref, bad)
            assert np.max(np.abs(bad - ref)) > 0, name
        ok = all(v <= 1 for v in worst.values())
        print("%-52s old tolerances %-7s bound %-7s worst err / bound: %s" % (
            name, "ACCEPT" if old else "reject", "ACCEPT" if ok else "reject", {k: "%.3g" % v for k, v in worst.items()}))
        assert not ok, "the bound accepts fault %s: %s" % (name, worst)
        if old:
            old_accepts.append(name)
    print("accepted by the old fixed tolerances: %s" % (old_accepts or "none"))
    assert len(faults) == 18


@pytest.mark.parametrize("fw", [45, 385, 512])
def test_width_bounds_hold_for_fp32_rounded_stages(fw):
    """The exact values pass, and so do fp32 roundings of every stage: the bound does not flag an evaluation a little less precise
    than the kernels'."""
    w = _weights(fw)
    v = _relu(fw, 2, 3 * fw)
    h = E.head_pair(v[0], v[1], w)
    B = E.head_bounds(h, w, "f32")
    h32 = E.head_pair(v[0], v[1], w, o1=h["o1"].astype(np.float32).astype(np.float64))
    worst = {k: E.ratio(h32[k], h[k], B[k]) for k in ("o2", "o3", "logit", "overlap")}
    c = E.corr_pair(v[0], v[1])
    worst["corr"] = E.ratio(c["corr"].astype(np.float32), c["corr"], c["direct"])
    print("W=%d fp32-rounded stages: worst err / bound %s" % (fw, {k: "%.3g" % x for k, x in worst.items()}))
    assert max(worst.values()) <= 1, worst
