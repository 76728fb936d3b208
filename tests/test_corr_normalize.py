"""CPU: NormalizedCorrelation2D's normalisations (`correlationHead_normalize`) and DeltaLayer's `negateDiffs` -- the fp64
restatement (tests/_corr_norm_ref.py) against the oracle's literal correlation, its edge channels, the `Infer` config check, and the
power of the elementwise bound the GPU tests use.

The bound (tests/_corr_norm_ref.corr_norm_pair).  The kernels store x~ = RN32(((x - m) + a) s), the affine form evaluated in fp64
and rounded once, with fp64 statistics.  Against the fp64 truth x' = ((x - m) + a) s (per-channel m, s of the exact formulas):
    |x~ - x'| <= sigma_n = u |x'| + 2^-44 s max|x| + U_SUB
(u = 2^-24 for the rounding; the fp64 sums behind m and s carry a few hundred fp64 roundings of |x|, far below 2^-44 |x|, and s
turns them into normalised units).  The correlation kernels then see the fp32 operands x~: their own error is E.corr_pair's bound
on those operands, which we evaluate on x' (the operands differ by sigma_n, a relative 2^-24 change of an fp32-level bound).  The
operand change itself moves corr[k] = sum_j sum_c l'[(k+j+180) mod 360, c] r'[j, c] by sum (l' dr + dl r') + O(d^2); the dl, dr are
independent roundings, so per shift they add in quadrature:
    sigma_k^2 = sum_j sum_c (l'^2 sigma_r^2 + sigma_l^2 r'^2)        (same index structure)
and B = E.corr_pair(l', r')[form] + SAFETY sigma_k, SAFETY = 6 as in oracle/error_bounds.py.  Nothing in it is fitted to results.
"""
import math

import numpy as np
import pytest

from oracle import error_bounds as E
from oracle import overlapnet_oracle as O
from overlapnet_amd import weights as WT
from tests import _corr_norm_ref as R
from tools import synthetic as S

NORM_MODES = ("euclidean", "scaling", "standardization")


def _lit(l, r, normalize="none"):
    return O.correlation_literal(np.asarray(l)[None, None], np.asarray(r)[None, None], normalize)[0, 0, :, 0]


def _pair(seed=0):
    rng = np.random.default_rng(seed + 10)
    l = R.edge_volume(seed)
    r = R.rolled(R.edge_volume(seed), 37) * np.float32(0.5) + np.maximum(rng.normal(0, 0.3, (360, 128)), 0).astype(np.float32)
    r[:, :8] = 0
    r[:, 8:18] = R.rolled(l[:, 8:18], 37)        # keep the edge channels exact on both sides
    return l, r


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------

def test_euclidean_equals_the_oracle_literal_form():
    l, r = _pair(0)
    ref = _lit(l, r, "euclidean")
    got = R.corr_norm_pair(l, r, "euclidean")["corr"]
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("mode", R.MODES)
def test_every_mode_equals_the_literal_form_on_normalised_volumes(mode):
    l, r = _pair(1)
    ref = _lit(R.normalize64(l, mode), R.normalize64(r, mode))
    got = R.corr_norm_pair(l, r, mode)["corr"]
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    # and the restatement of the normalisation is the formula of its docstring
    x = np.asarray(l, np.float64)
    if mode == "euclidean":
        want = x / np.sqrt(np.maximum((x * x).sum(axis=0), 1e-12))
    elif mode == "scaling":
        want = (x - x.min(axis=0)) / (x.max(axis=0) - x.min(axis=0) + 1e-6)
    elif mode == "standardization":
        y = (x - x.mean(axis=0)) + 1e-5
        want = y / np.sqrt(np.maximum((y * y).sum(axis=0), 1e-12))
    else:
        want = x
    np.testing.assert_allclose(R.normalize64(l, mode), want, rtol=1e-13, atol=0)


def test_reference_layer_demo():
    """The layer's own demo: W = 6, values 0..5, the right input rolled by one.  Under 'euclidean' the correlation peaks at 1 in
    bin 2 (the literal form and the restatement agree)."""
    l = np.arange(6, dtype=np.float32).reshape(6, 1)
    r = np.roll(l, 1, axis=0)
    c = _lit(l, r, "euclidean")
    assert int(np.argmax(c)) == 2 and abs(c[2] - 1.0) < 1e-15
    c2 = _lit(R.normalize64(l, "euclidean"), R.normalize64(r, "euclidean"))
    np.testing.assert_allclose(c2, c, rtol=1e-14)
    for mode in NORM_MODES:
        ln, rn = R.normalize64(l, mode), R.normalize64(r, mode)
        assert int(np.argmax(_lit(ln, rn))) == 2, mode


def _col(v, c, mode):
    return R.normalize64(v, mode)[:, c]


def test_edge_channels():
    v = R.edge_volume(0)
    inv = 1.0 / math.sqrt(360.0)
    # all zero
    for c in range(8):
        assert np.all(_col(v, c, "euclidean") == 0) and np.all(_col(v, c, "scaling") == 0)
        np.testing.assert_allclose(_col(v, c, "standardization"), inv, rtol=1e-12)
    # constant: the fp64 mean is exact, so standardization sees y = 1e-5 exactly
    np.testing.assert_allclose(_col(v, 8, "euclidean"), inv, rtol=1e-15)
    assert np.all(_col(v, 8, "scaling") == 0)
    np.testing.assert_allclose(_col(v, 8, "standardization"), inv, rtol=1e-12)
    # one non-zero column
    e = _col(v, 9, "euclidean")
    assert np.count_nonzero(e) == 1 and e.max() == 1.0
    assert abs(_col(v, 9, "scaling").max() - 2.5 / (2.5 + 1e-6)) < 1e-15
    assert abs(np.square(_col(v, 9, "standardization")).sum() - 1.0) < 1e-12
    # negative values; 2^100 (sum x^2 ~ 2^207 overflows fp32 but not fp64); 2^-100 and subnormals (sum x^2 < 1e-12: scaled by 1e6)
    for c in (10, 11, 12, 13):
        for mode in ("euclidean", "standardization"):
            if c != 13 or mode == "standardization":      # 2^-100 under euclidean: sum x^2 < 1e-12, not a unit vector
                assert abs(np.square(_col(v, c, mode)).sum() - 1.0) < 1e-12, (c, mode)
        sc = _col(v, c, "scaling")
        assert sc.min() == 0 and sc.max() <= 1.0
    assert np.all(np.isfinite(R.normalize32(v, "euclidean")))
    np.testing.assert_array_equal(_col(v, 13, "euclidean"), v[:, 13].astype(np.float64) * 1e6)
    np.testing.assert_array_equal(_col(v, 14, "euclidean"), v[:, 14].astype(np.float64) * 1e6)
    assert np.all(R.normalize32(v, "euclidean")[:, 14] > 0)       # the subnormals come out as normal fp32 values
    # the +1e-6 of scaling decides a channel whose range is below it; the +1e-5 of standardization one whose values are below it
    assert _col(v, 15, "scaling").max() < 0.25
    st = _col(v, 16, "standardization")
    assert st.min() > 0 and st.max() / st.min() < 1.5
    # the stored fp32 values are within the elementwise sigma_n of the bound
    for mode in R.MODES:
        err = np.abs(R.normalize32(v, mode).astype(np.float64) - R.normalize64(v, mode))
        assert np.all(err <= R.norm_sigma(v, mode)), mode


# ---- 2. Infer config validation ----------------------------------------------------------------------------------------------------

def _cfg(**model):
    cfg = {"model": dict({"leg_output_width": 360, "inputShape": [64, 900], "legsType": "360OutputkLegs",
                          "overlap_head": "DeltaLayerConv1NetworkHead", "orientation_head": "CorrelationHead"}, **model),
           "infer_seqs": "07", "data_root_folder": "/nonexistent", "use_depth": True, "use_normals": True,
           "use_intensity": False, "use_class_probabilities": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    return cfg


@pytest.mark.parametrize("model", [{"correlationHead_normalize": "l2"}, {"correlationHead_normalize": "Euclidean"},
                                   {"correlationHead_normalize": None}, {"correlationHead_normalize": 1},
                                   {"deltaLayer_negateDiffs": "yes"}, {"deltaLayer_negateDiffs": 1},
                                   {"deltaLayer_negateDiffs": None}])
def test_infer_rejects_unknown_head_options(model):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd._lib import OvnError
    with pytest.raises(ValueError) as ei:
        Infer(_cfg(**model))
    assert not isinstance(ei.value, OvnError)
    assert ("correlationHead_normalize" in str(ei.value)) or ("deltaLayer_negateDiffs" in str(ei.value))


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("negate", [False, True])
def test_valid_head_options_pass_validation(mode, negate):
    # a value built at run time (not an interned literal): compared by value, unlike the reference's `is`
    m = "".join(list(mode))
    assert WT.head_options({"correlationHead_normalize": m, "deltaLayer_negateDiffs": negate}) == (mode, negate)
    assert WT.head_options({}) == ("none", False)
    assert WT.head_options({"deltaLayer_negateDiffs": np.bool_(True)}) == ("none", True)


def test_valid_head_options_reach_the_engine():
    """With valid keys Infer gets past the check to the engine: on a GPU-less host that is the library's OvnError (no GPU), not the
    option error."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("checks the path up to the engine on a host without a GPU")
    from overlapnet_amd.infer import Infer
    from overlapnet_amd._lib import OvnError
    for mode in R.MODES:
        with pytest.raises(OvnError):
            Infer(_cfg(correlationHead_normalize=mode, deltaLayer_negateDiffs=True))


# ---- 3. gate power -----------------------------------------------------------------------------------------------------------------

def _corr64(l, r):
    return E.corr_pair(np.asarray(l, np.float64), np.asarray(r, np.float64))["corr"]


def _fault_volumes(v, mode, fault):
    """The normalised volume a faulty kernel would produce (fp32)."""
    x = np.asarray(v, np.float64)
    if fault == "over_channels":
        return R.normalize32(x.T, mode).T if mode != "scaling" else _scaling_axis(x, axis=1)
    if fault == "mean_of_squares":
        m, a, _ = R.affine64(x, mode)
        y = (x - m) + a
        return (y / np.sqrt(np.maximum(np.square(y).mean(axis=0, keepdims=True), 1e-12))).astype(np.float32)
    if fault == "constant_dropped":
        if mode == "scaling":
            with np.errstate(invalid="ignore", divide="ignore"):
                return ((x - x.min(axis=0)) / (x.max(axis=0) - x.min(axis=0))).astype(np.float32)
        y = x - x.mean(axis=0)
        return (y / np.sqrt(np.maximum(np.square(y).sum(axis=0), 1e-12))).astype(np.float32)
    if fault == "min_max_swapped":
        return ((x - x.max(axis=0)) / (x.min(axis=0) - x.max(axis=0) + 1e-6)).astype(np.float32)
    raise ValueError(fault)


def _scaling_axis(x, axis):
    lo, hi = x.min(axis=axis, keepdims=True), x.max(axis=axis, keepdims=True)
    return ((x - lo) / (hi - lo + 1e-6)).astype(np.float32)


CORR_FAULTS = [("over_channels", m) for m in NORM_MODES] + [("mean_of_squares", "euclidean"), ("mean_of_squares", "standardization"),
                                                             ("constant_dropped", "scaling"), ("constant_dropped", "standardization"),
                                                             ("min_max_swapped", "scaling")] + [("one_side_only", m) for m in NORM_MODES]


@pytest.mark.parametrize("mode", R.MODES)
def test_bound_accepts_the_correct_fp32_normalisation(mode):
    """The kernels' arithmetic emulated: fp32-rounded normalised operands, the correlation of those in fp64 and rounded to fp32.
    Both bound forms accept it (the worst ratio is printed)."""
    for seed in (0, 1):
        l, r = _pair(seed)
        if mode == "none":                 # unnormalised, 2^100 x 2^100 is beyond fp32: that channel is left out
            l[:, 12], r[:, 12] = 0, 0
        ref = R.corr_norm_pair(l, r, mode)
        got = _corr64(R.normalize32(l, mode), R.normalize32(r, mode)).astype(np.float32)
        for form in ("direct", "spectral"):
            rat = E.ratio(got, ref["corr"], ref[form])
            print("[%s seed %d %s] worst err / bound %.3g" % (mode, seed, form, rat))
            assert rat <= 1.0, (mode, seed, form, rat)


@pytest.mark.parametrize("fault,mode", CORR_FAULTS)
def test_bound_rejects_every_normalisation_fault(fault, mode):
    l, r = _pair(0)
    ref = R.corr_norm_pair(l, r, mode)
    if fault == "one_side_only":
        bad = _corr64(R.normalize32(l, mode), r)
    else:
        bad = _corr64(_fault_volumes(l, mode, fault), _fault_volumes(r, mode, fault))
    rat = min(E.ratio(bad, ref["corr"], ref["direct"]), E.ratio(bad, ref["corr"], ref["spectral"]))
    print("[%s %s] err / bound %.3g" % (fault, mode, rat))
    assert rat > 1.0, (fault, mode, rat)


@pytest.mark.parametrize("mode", NORM_MODES)
def test_head_bound_rejects_the_mode_applied_to_the_delta_head(mode):
    """Only the correlation head normalises: a Delta head fed the normalised volumes fails the head's bounds (every head mode)."""
    w = S.make_test_weights(4, seed=0)
    sc = E.value_edge_sets()["single_column"]
    l, r = sc[4], sc[0]                     # O(1) ReLU volumes with dead channels
    ref = E.head_pair(l, r, w)
    bad = E.head_pair(R.normalize32(l, mode), R.normalize32(r, mode), w)
    for hm in ("f16x3", "bf16x3", "f32"):
        B = E.head_bounds(ref, w, hm)
        rat = max(E.ratio(bad[k], ref[k], B[k]) for k in ("o2", "logit"))
        print("[%s %s] worst err / bound %.3g" % (mode, hm, rat))
        assert rat > 1.0, (mode, hm, rat)

