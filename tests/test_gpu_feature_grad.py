"""GPU (MI355X): both heads' losses differentiated down to the feature volumes (`ovn_heads_feature_grad`,
csrc/heads_feature_grad.hip) and `train.heads_loss` on top of it, against the fp64 restatement of tests/_feature_grad_ref.py.

Geometries (W, s), as tests/test_gpu_head_train.py: (45, 15) G = 3, odd W (half width 22); (60, 15) overlapping taps; (77, 15)
R = 75 < W: rows 75, 76 get only the yaw part, R is no multiple of 16, odd W; (50, 16) and (45, 10): s != 15; (360, 15): two pairs.
Pair counts 1, 3 and OVN_GRAD_PAIR_BLOCK + 1, index lists with repeats and the 1-vs-N form, both overlap losses; every case runs
overlap-only (yaw_bins None), yaw-only (overlap_scale 0) and both.

Per case
  1. the ReLU masks of the GPU's forward (the o2 / o3 of `delta_head_grad` on the same pairs: the same forward, and its overlap
     and head gradients must equal this call's bit for bit) equal fp64's except within the fp32 bound of zero, and are then forced
     into the reference; dfeat_l and dfeat_r of each of the three runs stay within 4 T of fp64, T = max |g32 - g64| of the same
     restatement in float32 on the CPU.
     corr within 2 u sum |terms| of the fp64 logits, u = 2^-24.  Derivation: the kernel sums the exact fp64 products of the fp32
     operands in fp64 and rounds once to fp32: |fl32(z') - z| <= u |z'| + |z' - z|, |z' - z| <= (W 128 + 6) 2^-53 sum |terms|
     < 2^-36 sum |terms|, |z'| <= (1 + 2^-36) sum |terms|; together below (u + 2^-35) sum |terms|: the constant 2 is generous.
     loss_yaw within yaw_scale x mean over (p, k) of |d loss / d z| x that bound, plus 4 u |loss|.
  2. structure: overlap-only rows >= R are exactly 0; the rows of the pair whose left and right are one volume of equal rows (every
     l[i, c] - r[j, c] is 0, so every sign is; note that lidx == ridx alone does not do that: l[i, c] - l[j, c] != 0 for i != j)
     are exactly 0; overlap_scale 0 gives zero head gradients and L_ov = 0; yaw_bins None and yaw_scale 0 give the same bits and
     L_yaw = 0.
  3. the same call twice, and the call cut into chunks of one pair block, give the same bits in every output.
With OVN_FEATURE_GRAD_PARITY_JSON set, the measured ratios max |g_gpu - g64| / T per tensor, run and case are written to that file."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from tests import _feature_grad_ref as F
from tests import _head_grad_ref as R

pytestmark = pytest.mark.gpu

_RATIOS = {}
OV_SCALE, YAW_SCALE = 5.0, 1.0
PARTS = ("overlap", "yaw", "both")
OUT_KEYS = ("dfeat_l", "dfeat_r", "loss", "overlap", "corr", "flat")


def _engine(W, s, weights, load=True, **model_extra):
    from overlapnet_amd.engine import OvnEngine
    h, wi = R.GEOMS[(W, s)]
    e = OvnEngine(h, wi, 4)
    try:
        if load:
            e.load_weights(weights, dict(R.model_cfg(W, s), **model_extra))
            assert e.feat_w == W and e.conv1size == s
    except Exception:
        e.close()
        raise
    return e


@pytest.fixture(scope="module")
def parity_file():
    yield
    path = os.environ.get("OVN_FEATURE_GRAD_PARITY_JSON")
    if path and _RATIOS:
        worst = max(max(v.values()) for v in _RATIOS.values())
        with open(path, "w") as f:
            json.dump({"what": "max |g_gpu - g64| / max |g32_cpu - g64| per tensor and run (pass: <= 4)", "worst": worst,
                       "cases": _RATIOS}, f, indent=1, sort_keys=True)


def _pools(eng, c):
    return torch.from_numpy(c["pool"]).to(eng.device), torch.from_numpy(c["right"]).to(eng.device)


def _call(eng, c, part, bins=None, targets=None, **kw):
    pool, right = _pools(eng, c)
    args = dict(lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"], overlap_scale=0.0 if part == "yaw" else OV_SCALE,
                yaw_scale=YAW_SCALE, want_head_grads=True)
    args.update(kw)
    yb = None if part == "overlap" else (c["bins"] if bins is None else bins)
    return eng.heads_feature_grad(pool, right, c["targets"] if targets is None else targets, yb, **args)


def _same(a, b, what):
    for k in OUT_KEYS:
        assert torch.equal(a[k], b[k]), "%s: %s" % (what, k)


def _corr_bound(c):
    la, ra = torch.tensor(np.abs(c["l"]), dtype=torch.float64), torch.tensor(np.abs(c["r"]), dtype=torch.float64)
    return 2.0 * E.U32 * F.corr_logits(la, ra).numpy()


def _ratio(gpu, g32, g64):
    T = float(np.max(np.abs(g32.astype(np.float64) - g64)))
    err = float(np.max(np.abs(gpu.astype(np.float64) - g64)))
    return T, err, (err / T if T > 0 else (0.0 if err == 0 else float("inf")))


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_feature_gradients_against_fp64(case, parity_file):
    W, s, n, form, loss = case
    Rr = (W // s) * s
    c, ref = F.reference(case, grad=False)
    eng = _engine(W, s, c["weights"])
    try:
        pool, right = _pools(eng, c)
        head = eng.delta_head_grad(pool, right, c["targets"], lidx=c["lidx"], ridx=c["ridx"], loss=loss, scale=OV_SCALE,
                                   want_activations=True)
        outs = {part: _call(eng, c, part) for part in PARTS}
        # 3. determinism and chunking
        for part in PARTS:
            _same(outs[part], _call(eng, c, part), part + " twice")
        if n > R.PAIR_BLOCK:
            eng.set_head_pipeline(chunk_pairs=R.PAIR_BLOCK)
            for part in PARTS:
                _same(outs[part], _call(eng, c, part), part + " chunked")
            eng.set_head_pipeline()
        # 2. structure
        _same(outs["overlap"], _call(eng, c, "both", yaw_scale=0.0), "yaw_scale 0 against yaw_bins None")
        no_heads = _call(eng, c, "both", want_head_grads=False)
        assert "flat" not in no_heads
        for k in OUT_KEYS[:-1]:
            assert torch.equal(no_heads[k], outs["both"][k]), "without head_grad_dev: " + k
        for part in ("overlap", "both"):
            assert torch.equal(outs[part]["flat"], head["flat"]), part
            assert torch.equal(outs[part]["loss"][0], head["loss"][0]), part
        for part in PARTS:
            assert torch.equal(outs[part]["overlap"], head["overlap"]), part
        assert not torch.any(outs["yaw"]["flat"]) and float(outs["yaw"]["loss_overlap"]) == 0.0
        assert float(outs["overlap"]["loss_yaw"]) == 0.0
        got = {part: {k: v.cpu().numpy() for k, v in outs[part].items() if isinstance(v, torch.Tensor)} for part in PARTS}
        o2, o3 = head["o2"].cpu().numpy(), head["o3"].cpu().numpy()
    finally:
        eng.close()
    for k in ("dfeat_l", "dfeat_r"):
        assert not np.any(got["overlap"][k][:, Rr:]), k
        if case == F.SELF_PAIR_CASE:
            assert not np.any(got["overlap"][k][1]), k
            assert np.any(got["both"][k][1]), k
    # 1. same linear region, then the gradients on the branch the GPU took
    und = R.undecided(c, ref)
    masks = []
    for k, pre, act in (("o2", "pre2", o2), ("o3", "pre3", o3)):
        m = act > 0
        differ = m != (ref[pre] > 0)
        print("%s: %d of %d signs differ, %d units undecided" % (k, differ.sum(), differ.size, und[k].sum()))
        assert not np.any(differ & ~und[k]), k
        assert und[k].mean() <= 1e-3
        masks.append(m)
    kw = dict(overlap_scale=OV_SCALE, yaw_scale=YAW_SCALE, masks=masks)
    ref64 = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], c["bins"], s, loss, **kw)
    ref32 = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], c["bins"], s, loss, dtype=torch.float32, **kw)
    ratios = {}
    for part in PARTS:
        for key, name in (("dl", "dfeat_l"), ("dr", "dfeat_r")):
            g64 = ref64[key][part]
            assert got[part][name].shape == g64.shape
            T, err, ratio = _ratio(got[part][name], ref32[key][part], g64)
            ratios["%s/%s" % (name, part)] = ratio
            print("%-8s %-8s max|g64| %.3e  T %.3e  gpu err %.3e  ratio %.3f" % (name, part, np.abs(g64).max(), T, err, ratio))
    _RATIOS["-".join(str(v) for v in case)] = ratios
    cb = _corr_bound(c)
    slope = np.abs(ref64["dz"]) * (n * W / YAW_SCALE)                     # |d loss / d z| per logit
    lbound = YAW_SCALE * float((slope * cb).mean()) + 4 * E.U32 * abs(ref64["loss_yaw"])
    for part in PARTS:
        cerr = np.abs(got[part]["corr"].astype(np.float64) - ref64["z"])
        print("%-8s corr err / bound %.3f" % (part, float(np.max(cerr / cb))))
        assert np.all(cerr <= cb), part
    for part in ("yaw", "both"):
        lerr = abs(float(got[part]["loss"][1]) - ref64["loss_yaw"])
        print("%-8s loss_yaw err %.3e bound %.3e" % (part, lerr, lbound))
        assert lerr <= lbound, part
    for k, v in ratios.items():
        assert v <= 4.0, (k, v)


def test_negated_differences():
    """deltaLayer_negateDiffs: the library holds the negated kernel and uses it as registered; the reference negates the differences."""
    case = (45, 15, 5, "idx", "sigmoid")
    c = F.make_case(case)
    eng = _engine(45, 15, c["weights"], deltaLayer_negateDiffs=True)
    try:
        pool, right = _pools(eng, c)
        head = eng.delta_head_grad(pool, right, c["targets"], lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"], scale=OV_SCALE,
                                   want_activations=True)
        out = _call(eng, c, "both")
        got = {k: out[k].cpu().numpy() for k in ("dfeat_l", "dfeat_r")}
        masks = [head["o2"].cpu().numpy() > 0, head["o3"].cpu().numpy() > 0]
    finally:
        eng.close()
    kw = dict(overlap_scale=OV_SCALE, yaw_scale=YAW_SCALE, masks=masks, negate=True)
    ref64 = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], c["bins"], 15, c["loss"], **kw)
    ref32 = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], c["bins"], 15, c["loss"], dtype=torch.float32, **kw)
    for key, name in (("dl", "dfeat_l"), ("dr", "dfeat_r")):
        T, err, ratio = _ratio(got[name], ref32[key]["both"], ref64[key]["both"])
        print("%-8s T %.3e gpu err %.3e ratio %.3f" % (name, T, err, ratio))
        assert ratio <= 4.0, name
        flipped = F.reference(case)[1][key]["both"]                    # the un-negated head's: the sign matters
        assert np.max(np.abs(ref64[key]["both"] - flipped)) > 100 * T


def test_heads_loss_autograd():
    """`train.heads_loss` at (60, 15) with index lists that repeat entries: the pools are a * pool for a leaf a (k, 1, 1) of ones."""
    from overlapnet_amd.train import heads_loss
    case = (60, 15, 5, "idx", "sigmoid")
    c = F.make_case(case)
    assert len(set(c["lidx"])) < 5
    eng = _engine(60, 15, c["weights"])
    try:
        pool, _ = _pools(eng, c)
        results = []
        for _ in range(2):
            a = torch.ones((pool.shape[0], 1, 1), device=eng.device, requires_grad=True)
            x = a * pool
            total = heads_loss(eng, x, x, c["targets"], c["bins"], lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"],
                               overlap_scale=OV_SCALE, yaw_scale=YAW_SCALE)
            assert total.dim() == 0 and total.requires_grad
            total.backward()
            results.append((total.detach().clone(), a.grad.detach().clone()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
        out = _call(eng, c, "both")
        assert torch.equal(results[0][0], out["loss_overlap"] + out["loss_yaw"])
        head = eng.delta_head_grad(pool, pool, c["targets"], lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"], scale=OV_SCALE,
                                   want_activations=True)
        masks = [head["o2"].cpu().numpy() > 0, head["o3"].cpu().numpy() > 0]
        ga = results[0][1].reshape(-1).cpu().numpy()
    finally:
        eng.close()
    args = (c["weights"], c["pool"], c["lidx"], c["ridx"], c["targets"], c["bins"], 15, c["loss"], OV_SCALE, YAW_SCALE)
    _, g64 = F.pool_scale_grad(*args, masks=masks)
    _, g32 = F.pool_scale_grad(*args, dtype=torch.float32, masks=masks)
    T, err, ratio = _ratio(ga, g32, g64)
    print("a.grad %s  fp64 %s  T %.3e gpu err %.3e ratio %.3f" % (ga, g64, T, err, ratio))
    assert np.abs(g64).max() > 1e-3
    assert ratio <= 4.0


def test_bins_out_of_range_give_an_all_zero_target():
    """A bin outside [0, W) on one pair: every other pair keeps its bits, that pair's yaw part equals the bits of the same pair put
    under the threshold, and both gradients stay within 4 T of the fp64 reference built with q = 0 for that pair (the GPU's ReLU
    masks forced, T from the float32 restatement, as in the parity test); loss_yaw within its bound of that reference's."""
    case = (45, 15, 5, "1vN", "mse")
    c = F.make_case(case)
    hot = int(np.flatnonzero(c["targets"] > F.THRESHOLD)[0])           # a pair whose bin counts
    eng = _engine(45, 15, c["weights"])
    try:
        base = _call(eng, c, "both")
        pool, right = _pools(eng, c)
        head = eng.delta_head_grad(pool, right, c["targets"], lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"], scale=OV_SCALE,
                                   want_activations=True)
        masks = [head["o2"].cpu().numpy() > 0, head["o3"].cpu().numpy() > 0]
        # the fp64 reference built with q = 0 for that pair, and the same in float32 for T (the rule of the parity test)
        qbins = np.array(c["bins"], np.int64)
        qbins[hot] = -1
        kw = dict(overlap_scale=OV_SCALE, yaw_scale=YAW_SCALE, masks=masks)
        ref = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], qbins, 15, c["loss"], **kw)
        ref32 = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], qbins, 15, c["loss"], dtype=torch.float32, **kw)
        assert not ref["q"][hot].any()
        with_bin = F.feature_loss(c["weights"], c["l"], c["r"], c["targets"], c["bins"], 15, c["loss"], **kw)
        low = np.array(c["targets"], np.float32)
        low[hot] = 0.5                                                 # the same pair with q = 0 by the threshold: the overlap loss changes too,
        want_yaw = _call(eng, c, "yaw", targets=low)                   # so compare the yaw-only runs
        for bad in (-1, 45, 2 ** 31 - 1, -2 ** 31):
            bins = np.array(c["bins"], np.int64)
            bins[hot] = bad
            out = _call(eng, c, "both", bins=bins.astype(np.int32))
            outy = _call(eng, c, "yaw", bins=bins.astype(np.int32))
            keep = [p for p in range(5) if p != hot]
            for k in ("dfeat_l", "dfeat_r", "corr", "overlap"):
                assert torch.equal(out[k][keep], base[k][keep]), (bad, k)
            assert not torch.equal(out["dfeat_l"][hot], base["dfeat_l"][hot])
            for k in ("dfeat_l", "dfeat_r", "corr"):
                assert torch.equal(outy[k][hot], want_yaw[k][hot]), (bad, k)
            for key, name in (("dl", "dfeat_l"), ("dr", "dfeat_r")):
                T, err, ratio = _ratio(out[name].cpu().numpy(), ref32[key]["both"], ref[key]["both"])
                print("bin %d %-8s T %.3e gpu err %.3e ratio %.3f" % (bad, name, T, err, ratio))
                assert ratio <= 4.0, (bad, name)
                # the bin matters: the reference that keeps it lies far outside that bound
                assert np.max(np.abs(ref[key]["both"][hot] - with_bin[key]["both"][hot])) > 100 * T, name
            slope = np.abs(ref["dz"]) * (5 * 45 / YAW_SCALE)
            lbound = YAW_SCALE * float((slope * _corr_bound(c)).mean()) + 4 * E.U32 * abs(ref["loss_yaw"])
            assert abs(float(out["loss_yaw"]) - ref["loss_yaw"]) <= lbound
            assert abs(float(out["loss_yaw"]) - float(base["loss_yaw"])) > 1e-3
    finally:
        eng.close()


def test_argument_and_state_errors():
    from overlapnet_amd._lib import OvnError
    c = F.make_case((45, 15, 3, "idx", "mse"))
    eng = _engine(45, 15, c["weights"])
    bare = _engine(45, 15, c["weights"], load=False)
    try:
        pool, _ = _pools(eng, c)
        kw = dict(lidx=c["lidx"], ridx=c["ridx"])
        with pytest.raises(ValueError):
            eng.heads_feature_grad(pool, pool, c["targets"], c["bins"], loss="hinge", **kw)
        for name in ("overlap_scale", "yaw_scale", "min_overlap_for_angle"):
            with pytest.raises(ValueError):
                eng.heads_feature_grad(pool, pool, c["targets"], c["bins"], **dict(kw, **{name: float("inf")}))
        with pytest.raises(IndexError):
            eng.heads_feature_grad(pool, pool, c["targets"], c["bins"], lidx=[0, 1, 99], ridx=c["ridx"])
        with pytest.raises(OvnError):
            eng.heads_feature_grad(pool, pool, c["targets"][:2], c["bins"], **kw)
        with pytest.raises(OvnError):
            eng.heads_feature_grad(pool, pool, c["targets"], c["bins"][:2], **kw)
        # the C entry point: outputs filled with a sentinel stay untouched (the error comes before the first launch)
        dev = eng.device
        d = torch.full((2, 3, 45, 128), 7.0, device=dev)
        t = torch.from_numpy(c["targets"]).to(dev)
        b = torch.from_numpy(c["bins"]).to(dev)
        lossv = torch.full((2,), 7.0, device=dev)
        p = lambda x: None if x is None else C.c_void_p(x.data_ptr())      # noqa: E731

        def call(h, feats=pool, n=3, target=t, bins=b, loss=0, so=5.0, sy=1.0, thr=0.7, dl=d[0], dr=d[1], lv=lossv):
            return eng.lib.ovn_heads_feature_grad(h, p(feats), None, p(feats), None, n, p(target), p(bins), loss, so, sy, thr, p(dl),
                                                  p(dr), None, p(lv), None, None, None)
        for kwargs in (dict(feats=None), dict(target=None), dict(dl=None), dict(dr=None), dict(lv=None), dict(n=0), dict(n=-4),
                       dict(loss=2), dict(loss=-1), dict(so=float("nan")), dict(sy=float("inf")), dict(thr=float("nan"))):
            assert call(eng._h, **kwargs) == 1, kwargs
        assert call(None) == 1
        assert call(bare._h) == 3 and b"head weights" in eng.lib.ovn_last_error()
        eng.set_corr_normalization("euclidean")
        assert call(eng._h) == 3 and b"normalisation" in eng.lib.ovn_last_error()
        with pytest.raises(OvnError):
            eng.heads_feature_grad(pool, pool, c["targets"], c["bins"], **kw)
        torch.cuda.synchronize()
        assert bool(torch.all(d == 7.0)) and bool(torch.all(lossv == 7.0))
        ok = eng.heads_feature_grad(pool, pool, c["targets"], None)            # no yaw part: any normalisation mode will do (1-vs-N)
        eng.set_corr_normalization("none")
        assert call(eng._h, bins=None) == 0 and call(eng._h, sy=0.0) == 0
        torch.cuda.synchronize()
        assert float(lossv[1]) == 0.0 and torch.equal(d[0], ok["dfeat_l"]) and torch.equal(d[1], ok["dfeat_r"])
    finally:
        eng.close()
        bare.close()
