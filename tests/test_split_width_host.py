"""CPU: the split (f16x3) Delta head at feature widths other than 360 -- its error bound, the faults that bound must reject, and
the public surface (both exports, the binding, the `width_precision` key of Infer).

The bound is `oracle/error_bounds.head_bounds(h, w, "f16x3")` on a `head_pair` result to which tests/_split_width_ref.py adds the
min-form entry the oracle leaves out off 360.  Faults are built as the c_conv1 output a faulty kernel would produce and pushed
through the rest of the head in fp64 (`head_pair(..., o1=)`), as tests/test_error_bound_width.py does."""
import os
import re

import numpy as np
import pytest

from oracle import error_bounds as E
from tests import _split_width_ref as SR
from tools import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_WIDTHS = (45, 59, 385, 422, 512)
STAGES = ("o2", "o3", "logit", "overlap")
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


# ---- the helper is the oracle's own entry at 360, and a bound at every other width ------------------------------------------------

def test_min_entry_equals_the_oracle_at_360():
    w = _weights(360)
    v = _relu(360, 2, 7)
    v[1][5, 3] = np.float32(-0.75)                                # a shifted pair
    val, rms = SR.min_entry(v[0], v[1], w)
    oval, orms = E.head_pair(v[0], v[1], w)["c1"]["min"]
    assert np.max(np.abs(val - oval)) <= 1e-12 * np.max(np.abs(oval))
    assert np.max(np.abs(rms - orms)) <= 1e-12 * np.max(np.abs(orms))


@pytest.mark.parametrize("fw", [45, 422, 512])
def test_f16x3_bound_exists_off_360_and_contains_the_exact_and_fp32_rounded_values(fw):
    w = _weights(fw)
    v = _relu(fw, 2, fw)
    h0 = E.head_pair(v[0], v[1], w)
    with pytest.raises(ValueError):                                # the oracle alone still has no f16x3 bound off 360
        E.head_bounds(h0, w, "f16x3")
    h = SR.head_pair_split(v[0], v[1], w)
    B, Bf = SR.bounds(h, w), E.head_bounds(h, w, "f32")
    assert all(np.all(np.asarray(B[k]) > 0) for k in ("o1", "o2", "o3", "logit"))
    assert np.all(B["o2"] >= Bf["o2"]) and B["logit"] >= Bf["logit"]          # the split bound is the wider one
    vm, va = h["c1"]["min"], h["c1"]["abs"]
    assert np.all(vm[0] >= va[0] * (1 - 1e-12)) and np.all(vm[1] >= va[1] * (1 - 1e-12))   # min form covers the abs form
    h32 = E.head_pair(v[0], v[1], w, o1=h["o1"].astype(np.float32).astype(np.float64))
    worst = {k: E.ratio(h32[k], h[k], B[k]) for k in STAGES}
    print("W=%d logit bound f16x3 %.3g (f32 %.3g), median o2 bound ratio %.3g, fp32-rounded o1: worst err / bound %s" % (
        fw, B["logit"], Bf["logit"], float(np.median(B["o2"] / Bf["o2"])), {k: "%.3g" % x for k, x in worst.items()}))
    assert max(worst.values()) <= 1 and all(E.ratio(h[k], h[k], B[k]) == 0 for k in STAGES)


# ---- fault models -----------------------------------------------------------------------------------------------------------------

def _c1_abs(l, r, w, transform=None):
    """c_conv1 (without bias) on transform(|l - r|), (W, G, 64), a few rows at a time."""
    l64, r64 = np.asarray(l, np.float64), np.asarray(r, np.float64)
    fw = l64.shape[0]
    g = fw // 15
    w1 = E._w(w, "c_conv1/kernel").reshape(15, 128, 64)
    out = np.empty((fw, g, 64))
    for i0 in range(0, fw, 32):
        d = np.abs(l64[i0:i0 + 32, None, :] - r64[None, :15 * g, :])
        out[i0:i0 + 32] = E._c1(d if transform is None else transform(d), w1, 15, fw)
    return out


def _fault_lo_hi_dropped(l, r, w, h):
    """The a_lo w_hi MFMA left out: hi = fp16_rtz(a) falls short of a by up to 2^-10 a, 2^-11 a on average, always downwards."""
    return E._w(w, "c_conv1/bias") + (h["o1"] - E._w(w, "c_conv1/bias")) * (1 - 2.0 ** -11)


def _fault_group_from_neighbour(l, r, w, h):
    """One column group's W1 x r tile computed from the rows of r of the group before it."""
    o1 = h["o1"].copy()
    jb = o1.shape[1] // 2
    o1[:, jb] = o1[:, jb - 1]
    return o1


def _fault_rows_leak(l, r, w, h):
    """Rows i >= R = 15 G of l are not dropped before the o1 image: they wrap onto its first W - R rows."""
    o1 = h["o1"].copy()
    fw = o1.shape[0]
    rr = 15 * (fw // 15)
    if fw == rr:
        return None
    o1[:fw - rr] = o1[rr:]
    return o1


def _fault_shift_forgotten(l, r, w, h):
    """The feature scale taken from the largest value instead of the shifted range max + c: |l - r| of a pair with negative values
    then exceeds fp16 in scaled units and the round-toward-zero conversion stops at 65504."""
    sa = E.pow2_scale(float(max(np.max(l), np.max(r))))
    return E._w(w, "c_conv1/bias") + _c1_abs(l, r, w, lambda d: np.minimum(d, 65504.0 / sa))


FAULTS = {"lo_hi_term_dropped": _fault_lo_hi_dropped, "column_group_from_its_neighbour": _fault_group_from_neighbour,
          "rows_beyond_R_leak_in": _fault_rows_leak, "shift_forgotten": _fault_shift_forgotten}


def _negative_pair(fw):
    v = _relu(fw, 2, 2 * fw + 1)
    rng = np.random.default_rng(fw)
    top = float(v.max())
    m = rng.random(v[1].shape) < 0.02
    v[1][m] = np.float32(-8.0 * top)                             # negative values well below -max: c = 8 max, span = 9 max
    return v


def test_bound_rejects_every_fault_and_accepts_the_exact_values():
    rejected = {k: [] for k in FAULTS}
    for fw in FAULT_WIDTHS:
        w = _weights(fw)
        for name, make in FAULTS.items():
            v = _negative_pair(fw) if name == "shift_forgotten" else _relu(fw, 2, fw)
            h = SR.head_pair_split(v[0], v[1], w)
            B = SR.bounds(h, w)
            assert all(E.ratio(h[k], h[k], B[k]) <= 1 for k in STAGES), (fw, name)      # the exact values sit inside
            o1 = make(v[0], v[1], w, h)
            if o1 is None:
                continue
            bad = E.head_pair(v[0], v[1], w, o1=o1)
            assert np.max(np.abs(bad["o2"] - h["o2"])) > 0, (fw, name)
            worst = {k: E.ratio(bad[k], h[k], B[k]) for k in STAGES}
            ok = all(x <= 1 for x in worst.values())
            print("W=%-3d %-34s bound %-6s worst err / bound %s" % (fw, name, "ACCEPT" if ok else "reject",
                                                                    {k: "%.3g" % x for k, x in worst.items()}))
            if not ok:
                rejected[name].append(fw)
    for name, ws in rejected.items():
        assert ws, "the f16x3 bound accepts fault %s at every width of %s" % (name, FAULT_WIDTHS)


# ---- header, binding, Infer key -----------------------------------------------------------------------------------------------------

def test_exports_are_declared_and_bound_and_the_abi_number_stays():
    import ctypes
    from overlapnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    assert re.search(r"\bint\s+ovn_set_head_width_split\s*\(\s*ovn_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+ovn_get_head_width_split\s*\(\s*ovn_ctx\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"#define\s+OVN_ABI_VERSION\s+11\b", src) and _lib.ABI_VERSION == 11
    assert _lib.SIGNATURES["ovn_set_head_width_split"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _lib.SIGNATURES["ovn_get_head_width_split"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)])
    lib = _lib.load()
    assert lib.ovn_abi_version() == 11
    assert lib.ovn_set_head_width_split(None, 1) == 1 and b"ctx is NULL" in lib.ovn_last_error()
    got = ctypes.c_int(7)
    assert lib.ovn_get_head_width_split(None, ctypes.byref(got)) == 1 and got.value == 7


def test_engine_surface():
    from overlapnet_amd.engine import OvnEngine, QueryAhead
    import inspect
    assert callable(OvnEngine.set_head_width_split)
    assert "set_head_width_split" in (OvnEngine.set_head_precision.__doc__ or "")
    assert "head_width_split" in inspect.getsource(QueryAhead)
    for k in ("delta_prep", "delta_c12", "delta_c2"):
        assert k in OvnEngine.PROFILE_KINDS


def _cfg(shape, fw, **extra):
    model = dict(S.REFERENCE_MODEL_CFG, inputShape=list(shape), leg_output_width=fw, additional_unsymmetric_layer3a=shape[0] == 64)
    cfg = {"model": model, "infer_seqs": "x",
           "data_root_folder": "/tmp", "use_depth": True, "use_normals": True, "use_class_probabilities": False,
           "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


class _Reached(Exception):
    pass


def _no_engine(monkeypatch, reach=False):
    from overlapnet_amd import infer as I

    def make(*a, **k):
        if reach:
            raise _Reached()
        raise AssertionError("an engine was created")
    monkeypatch.setattr(I, "OvnEngine", make)
    return I


@pytest.mark.parametrize("extra, what", [
    ({"width_precision": "fast"}, "must be 'exact' or 'split'"),
    ({"width_precision": "split", "precision": "f32"}, "needs config['precision'] = 'f16x3'"),
    ({"width_precision": "split", "precision": "bf16x3"}, "needs config['precision'] = 'f16x3'"),
])
def test_infer_refuses_the_key_before_any_engine(monkeypatch, extra, what):
    I = _no_engine(monkeypatch)
    with pytest.raises(Exception) as ei:
        I.Infer(_cfg((64, 1024), 422, **extra))
    assert what in str(ei.value)


@pytest.mark.parametrize("shape, fw, extra", [((64, 1024), 422, {"width_precision": "split"}),
                                              ((32, 900), 371, {"width_precision": "split", "precision": "f16x3"}),
                                              ((64, 900), 360, {"width_precision": "split"}),
                                              ((64, 1024), 422, {"width_precision": "exact", "precision": "f32"}),
                                              ((64, 1024), 422, {})])
def test_infer_accepts_the_key_up_to_the_engine(monkeypatch, shape, fw, extra):
    I = _no_engine(monkeypatch, reach=True)
    with pytest.raises(_Reached):
        I.Infer(_cfg(shape, fw, **extra))
