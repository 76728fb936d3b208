"""CPU: the elementwise error bounds (oracle/error_bounds.py) reject the faults a Delta-head kernel could have, where the old
north-star gates on the final outputs (|d overlap| <= 1e-4, |d logit| <= 1e-3 (1 + |logit|)) accept some of them.

Every fault is built from the fp64 oracle on the value-edge volumes the GPU tests use (`value_edge_sets`), as the c_conv1
output a faulty kernel would produce, and pushed through the rest of the head."""
import numpy as np
import pytest

from oracle import overlapnet_oracle as O

from oracle import error_bounds as E
from tools import synthetic as S

W = S.make_test_weights(4, seed=0)
SETS = E.value_edge_sets()


def _rtz16(x):
    """fp16 round-toward-zero hi part (the kernels' cvt_pkrtz for feature words)."""
    h = np.asarray(x, np.float64).astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(np.float64)


def _split(x, scale, hi_rtz):
    """(hi, lo) of x at a power-of-two scale, in true units: hi fp16 (rtz for features, rne for weights), lo = fp16(x - hi)."""
    xs = np.asarray(x, np.float64) * scale
    hi = _rtz16(xs) if hi_rtz else xs.astype(np.float16).astype(np.float64)
    lo = (xs - hi).astype(np.float16).astype(np.float64)
    return hi / scale, lo / scale


def _w1():
    return np.asarray(W["c_conv1/kernel"], np.float64).reshape(15, 128, 64)


def _min_form_o1(l, r, lo_weight):
    """c_conv1 in min form from split operands; lo_weight scales every lo plane (0: lost, 2: de-scaled one bucket too coarse)."""
    _, _, _, c = E.min_form_parts(l, r, W)
    lp, rp = np.asarray(l, np.float64) + c, np.asarray(r, np.float64) + c
    sa = E.pow2_scale(max(lp.max(), rp.max()))
    w1 = _w1()
    wh, wl = _split(w1, E.pow2_scale(np.abs(w1).max()), False)
    lh, ll = _split(lp, sa, True)
    rh, rl = _split(rp, sa, True)
    lq, rq = lh + lo_weight * ll, rh + lo_weight * rl
    x = lq[:, None, :] + rq[None, :, :] - 2 * np.minimum(lq[:, None, :], rq[None, :, :])
    return np.asarray(W["c_conv1/bias"], np.float64) + E._c1(x, wh + lo_weight * wl, 15)


def _o1_parts(l, r):
    lin_l, lin_r, M, c = E.min_form_parts(l, r, W)
    return np.asarray(W["c_conv1/bias"], np.float64) + lin_l + lin_r[None], M, c


def _fault_drop_channel_from_min_walk(l, r, ch):
    """A compacted walk that skips a live query channel: its min term is missing; the linear terms (TT, AA: the prepare and a2
    kernels, which walk all 128 channels) keep it."""
    base, M, c = _o1_parts(l, r)
    mn = np.minimum(l.astype(np.float64)[:, None, ch] + c, r.astype(np.float64)[None, :, ch] + c)     # (360, 360)
    Mch = np.einsum("ijd,do->ijo", mn.reshape(360, 24, 15), _w1()[:, ch, :])
    return base - 2 * (M - Mch)


def _fault_tap_shift(l, r, jb=23):
    """Column group jb = 23 reads its 15 right-hand columns one tap off (wrapping inside the group)."""
    o1 = E.head_pair(l, r, W)["o1"].copy()
    cols = 15 * jb + (np.arange(15) + 1) % 15
    d = np.abs(l.astype(np.float64)[:, None, :] - r.astype(np.float64)[None, cols, :])          # (360, 15, 128)
    o1[:, jb] = np.asarray(W["c_conv1/bias"], np.float64) + d.reshape(360, -1) @ _w1().reshape(-1, 64)
    return o1


def _fault_swap_channels_in_min_walk(l, r, a, b):
    """Two channels of the min walk paired with each other's W1 rows (a wrong entry of the packed slice's channel table)."""
    base, M, c = _o1_parts(l, r)
    w1 = _w1().copy()
    w1[:, [a, b]] = w1[:, [b, a]]
    lp, rp = l.astype(np.float64) + c, r.astype(np.float64) + c
    return base - 2 * E._c1(np.minimum(lp[:, None, :], rp[None, :, :]), w1, 15)


def _fault_no_shift_in_a2(l, r):
    """AA built from A2 = r W1 without the + c w1col term of a shifted pair."""
    _, _, _, c = E.min_form_parts(l, r, W)
    return E.head_pair(l, r, W)["o1"] - c * _w1().reshape(-1, 64).sum(axis=0)


def _packed_slice_channels(q):
    """The query's channel list as the kernels order it (build_chan_list: by the number of column-group pairs a channel is alive
    in, descending, ties in channel order) and the channels of its last 32-slot slice."""
    alive = (q.reshape(12, 30, 128) != 0).any(axis=1).sum(axis=0)
    live = [ch for ch in sorted(range(128), key=lambda ch: (-alive[ch], ch)) if alive[ch] > 0]
    return live[32 * ((len(live) - 1) // 32):]


def _faults():
    """(name, l, r, faulty o1) on the value-edge volumes; r is the query (the right-hand volume) of a 1-vs-N sweep."""
    sc = SETS["single_column"]
    tn = SETS["tiny_negative"]
    q15 = sc[1]                                        # 111 live channels: a packed last slice of 15
    last = _packed_slice_channels(q15)
    one_col = [ch for ch in last if np.count_nonzero(q15[:, ch]) == 1 and q15[:, ch].max() == 1.0]
    assert len(last) == 15 and len(one_col) >= 2
    neg = tn[0].copy()
    neg[17, 5] = np.float32(-0.5)
    return [
        ("lo_plane_lost", sc[4], q15, _min_form_o1(sc[4], q15, 0.0)),
        ("lo_plane_one_bucket_off", sc[4], q15, _min_form_o1(sc[4], q15, 2.0)),
        ("live_channel_dropped_from_min_walk", sc[4], q15, _fault_drop_channel_from_min_walk(sc[4], q15, one_col[0])),
        ("tap_shift_in_jb23", sc[4], sc[3], _fault_tap_shift(sc[4], sc[3])),
        ("channels_swapped_in_packed_slice", sc[4], q15, _fault_swap_channels_in_min_walk(sc[4], q15, one_col[0], one_col[1])),
        ("shift_missing_in_a2", tn[1], neg, _fault_no_shift_in_a2(tn[1], neg)),
    ]


def _old_gates(ref, bad):
    ov_ok = abs(bad["overlap"] - ref["overlap"]) <= 1e-4
    lg_ok = abs(bad["logit"] - ref["logit"]) <= 1e-3 * (1 + abs(ref["logit"]))
    return ov_ok and lg_ok


def _new_gate(ref, bad, mode):
    B = E.head_bounds(ref, W, mode)
    worst = {k: E.ratio(bad[k], ref[k], B[k]) for k in ("o2", "o3", "logit", "overlap")}
    return all(v <= 1 for v in worst.values()), worst


def test_bounds_hold_for_the_exact_values_and_fp32_roundings():
    """The oracle's own values pass; fp32-rounded operands of the same fp64 evaluation pass in every mode (an evaluation with a
    little less than the modes' precision is not flagged)."""
    l, r = SETS["single_column"][4], SETS["single_column"][0]
    ref = E.head_pair(l, r, W)
    for mode in ("f16x3", "bf16x3", "f32"):
        ok, worst = _new_gate(ref, ref, mode)
        assert ok and max(worst.values()) == 0
        o1 = ref["o1"].astype(np.float32).astype(np.float64)
        ok, worst = _new_gate(ref, E.head_pair(l, r, W, o1=o1), mode)
        print("[%s] fp32-rounded c_conv1 output: worst err / bound %s" % (mode, {k: "%.3g" % v for k, v in worst.items()}))
        assert ok, worst


def test_new_gate_rejects_every_fault_the_old_gates_accept_some():
    old_accepts = []
    for name, l, r, o1 in _faults():
        ref = E.head_pair(l, r, W)
        bad = E.head_pair(l, r, W, o1=o1)
        assert np.max(np.abs(bad["o1"] - ref["o1"])) > 0, name
        old = _old_gates(ref, bad)
        ok, worst = _new_gate(ref, bad, "f16x3")
        print("%-26s old gates %-7s new gate %-7s worst err / bound: %s" % (name, "ACCEPT" if old else "reject", "ACCEPT" if ok else "reject",
                                                                          {k: "%.3g" % v for k, v in worst.items()}))
        assert not ok, "the bound accepts fault %s: %s" % (name, worst)
        if old:
            old_accepts.append(name)
    assert len(old_accepts) >= 2, old_accepts


@pytest.mark.parametrize("s", [15, 10, 24])
def test_head_restatement_matches_the_oracle(s):
    """head_pair / corr_pair restate the oracle's heads stage by stage; the fault-power test rests on them."""
    from tools import synthetic as TS
    cfg = dict(TS.REFERENCE_MODEL_CFG, conv1NetworkHead_conv1size=s)
    w = TS.make_test_weights(4, seed=3, model_cfg=cfg) if s != 15 else W
    for name, i, j in (("neg_zero", 1, 0), ("tiny_negative", 2, 0), ("wide_range", 0, 1)):
        l, r = SETS[name][i], SETS[name][j]
        h = E.head_pair(l, r, w, s)
        _, lg, it = O.delta_head_forward(l[None, None], r[None, None], w, conv1size=s, return_intermediates=True)
        for k in ("o1", "o2", "o3"):
            assert np.max(np.abs(h[k] - it[k])) <= 1e-12 * (np.max(np.abs(it[k])) + 1e-300), (name, k)
        assert abs(h["logit"] - lg[0]) <= 1e-12 * (1 + abs(lg[0]))
        corr = O.correlation_head_forward(l[None, None], r[None, None])[0]
        assert np.max(np.abs(E.corr_pair(l, r)["corr"] - corr)) <= 1e-12 * np.max(np.abs(corr))


def test_spectral_corr_bound_rejects_a_zero_spectrum():
    """A subnormal volume's spectrum lost below the fp16 range (the correlation vector all zero) fails the spectral bound, as does a
    0.1 % error; the exact vector and fp32-rounded values pass."""
    for name, i in (("subnormal", 1), ("neg_zero", 1)):
        c = E.corr_pair(SETS[name][i], SETS[name][0])
        assert E.ratio(np.zeros(360), c["corr"], c["spectral"]) > 1e3
        assert E.ratio(c["corr"] * (1 + 1e-3), c["corr"], c["spectral"]) > 1
        assert E.ratio(c["corr"].astype(np.float32), c["corr"], c["spectral"]) < 0.2
