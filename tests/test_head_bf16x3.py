"""The bf16x3 head precision (`ovn_set_head_precision(ctx, 2)`, `OvnEngine.set_head_precision('bf16x3')`, `precision='bf16x3'`):
DeltaLayer + c_conv1 and c_conv2 on the bf16 matrix cores with every fp32 operand split exactly into three bf16 terms.

  1. operand resolution: a one-weight network whose c_conv2 output IS |l - r| on values that need 23 significand bits -- bf16x3 and
     f32 reproduce it exactly, f16x3 (22 bits) does not;
  2. parity at scale against the committed fp64-oracle goldens of test_parity_sweep.py (f32 leg + bf16x3 head), and against the f32 head
     on the same features;
  3. indexed pairs with negative values (the shift path) and the c_conv2 / c_conv3 activations against the fp64 oracle;
  4. the same bits across call forms, sweep sizes, pipelines and calls; 5. mode switching; 6. the API."""
import os

import numpy as np
import pytest
import torch

from oracle import overlapnet_oracle as O
from tools import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = S.REFERENCE_MODEL_CFG


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / (np.max(np.abs(b)) + 1e-30))


def _engine(C=4, w=None):
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, C)
    e.load_weights(S.make_test_weights(C, seed=0) if w is None else w, CFG)
    return e


def test_engine_and_infer_name_the_mode_without_a_gpu():
    """CPU: the Python side knows the mode (table, error message, docstrings)."""
    import inspect
    from overlapnet_amd import engine as E
    from overlapnet_amd import infer as I
    assert "'bf16x3'" in inspect.getsource(E.OvnEngine.set_head_precision)
    src = inspect.getsource(I.Infer.__init__)
    assert "'bf16x3'" in src and "'f16x3', 'f32' or 'bf16x3'" in src
    assert "bf16x3" in I.__doc__


def test_header_documents_mode_2():
    """CPU: the C header describes mode 2 and the ABI version moved with it."""
    from overlapnet_amd import _lib
    h = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    assert "#define OVN_ABI_VERSION %d" % _lib.ABI_VERSION in h and _lib.ABI_VERSION >= 7
    assert "2 = bf16x3" in h


# ---- 1. operand resolution -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
def test_operand_resolution_tells_24_bits_from_22():
    w = S.make_test_weights(4, seed=0)
    for k in ("c_conv1/kernel", "c_conv1/bias", "c_conv2/kernel", "c_conv2/bias"):
        w[k] = np.zeros_like(w[k])
    w["c_conv1/kernel"][0, 0, 0, 0] = 1.0    # W1[dj=0][c=0][o=0]
    w["c_conv2/kernel"][0, 0, 0, 0] = 1.0    # W2[di=0][o=0][p=0]
    rng = np.random.default_rng(5)
    # 1 + k 2^-22: l + r and l - r are exact in fp32; the values need 23 significand bits
    fv = (1.0 + rng.integers(0, 1 << 21, size=(2, 360, 128)) * 2.0 ** -22).astype(np.float32)
    l, r = fv[0].astype(np.float64), fv[1].astype(np.float64)
    want = np.abs(l[15 * np.arange(24)][:, None, 0] - r[15 * np.arange(24)][None, :, 0])   # [ib][jb]
    e = _engine(4, w)
    try:
        t = torch.from_numpy(fv).cuda()
        miss = {}
        for mode in ("bf16x3", "f32", "f16x3"):
            e.set_head_precision(mode)
            e.heads(t[:1], t[1:2])
            o2, _ = e.debug_head_activations(1)
            got = o2[0, :, :, 0].double().cpu().numpy()
            ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
            miss[mode] = float(np.mean(np.abs(got - want) > ulp))
            print("[%s] entries off by more than 1 ulp: %.3f, max |d| %.3g" % (mode, miss[mode], np.max(np.abs(got - want))))
        assert miss["bf16x3"] == 0.0 and miss["f32"] == 0.0, miss
        assert miss["f16x3"] > 0.1, miss     # the control: 22 bits per operand cannot resolve these values
    finally:
        e.close()


# ---- 2. parity at scale ----------------------------------------------------------------------------------------------------------
CASES = [("glorot", 4, 1024), ("trained_like", 4, 1024), ("trained_like", 1, 128), ("trained_like", 5, 128), ("trained_like", 4, 4096)]


def _golden(name, C, POOL):
    suffix = "" if (POOL, C) == (1024, 4) else "_c%d_p%d" % (C, POOL)
    with np.load(os.path.join(ROOT, "tests", "golden", "parity_sweep_%s%s.npz" % (name, suffix))) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
@pytest.mark.parametrize("wset,C,POOL", CASES)
def test_sweep_parity_f32_leg_bf16x3_head(wset, C, POOL):
    from overlapnet_amd.engine import OvnEngine
    g = _golden(wset, C, POOL)
    w = S.WEIGHT_SETS[wset](C)
    eng = OvnEngine(64, 900, C)
    eng.load_weights(w, CFG)
    try:
        fx = S.load_fixture_images()
        dev = eng.device
        eng.set_leg_precision("f32")
        cands = torch.empty((POOL, 360, 128), dtype=torch.float32, device=dev)
        for s, imgs in S.sweep_pool_images(POOL, C, 0, fx):
            eng.leg(torch.from_numpy(imgs).to(dev), out=cands[s:s + imgs.shape[0]])
        qfv = eng.leg(torch.from_numpy(S.sweep_query_image(C, fx)).to(dev))
        res = {}
        for mode in ("bf16x3", "f32", "f16x3"):
            eng.set_head_precision(mode)
            r = eng.heads(cands, qfv, spec_l=eng.spectrum(cands), spec_r=eng.spectrum(qfv), want_logit=True)
            res[mode] = {k: r[k].cpu().numpy() for k in ("overlap", "logit", "yaw")}
        d = {m: np.abs(res[m]["overlap"].astype(np.float64) - g["overlap"]) for m in res}
        print("[%s C%d P%d] max |d overlap| vs fp64: bf16x3 %.3g  f32 %.3g  f16x3 %.3g;  |bf16x3 - f32| %.3g  |f16x3 - f32| %.3g" %
              (wset, C, POOL, d["bf16x3"].max(), d["f32"].max(), d["f16x3"].max(),
               np.max(np.abs(res["bf16x3"]["overlap"] - res["f32"]["overlap"])), np.max(np.abs(res["f16x3"]["overlap"] - res["f32"]["overlap"]))))
        b = res["bf16x3"]
        assert d["bf16x3"].max() <= 1e-4
        assert np.all(np.abs(b["logit"] - g["logit"]) <= 1e-3 * (1 + np.abs(g["logit"])))
        bad = np.nonzero(b["yaw"] != g["yaw"])[0]
        assert not [i for i in bad if g["corr_top2_gap"][i] > 1e-5], bad
        assert d["bf16x3"].max() <= 1.5 * d["f32"].max() + 1e-6, (d["bf16x3"].max(), d["f32"].max())
    finally:
        eng.close()


# ---- 3. indexed pairs, negative values, intermediates -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
def test_indexed_signed_pairs_and_intermediates_against_oracle():
    rng = np.random.default_rng(23)
    fv = rng.normal(0.0, 1.0, size=(5, 360, 128)).astype(np.float32)       # signed: every pair takes the shift
    fv[2] *= 300.0
    fv[4] = np.maximum(rng.normal(0.3, 1.0, size=(360, 128)), 0)           # ReLU-like: the pair (4, 4) needs no shift
    w = S.make_test_weights(4, seed=0)
    pairs = np.array([[0, 1], [2, 0], [1, 2], [3, 3], [4, 4], [4, 1]])
    fv4 = fv.reshape(-1, 1, 360, 128).astype(np.float64)
    ov, yaw, lg, corr = O.heads_forward(fv4[pairs[:, 0]], fv4[pairs[:, 1]], w)
    e = _engine(4, w)
    try:
        e.set_head_precision("bf16x3")
        t = torch.from_numpy(fv).cuda()
        r = e.heads(t, t, lidx=pairs[:, 0], ridx=pairs[:, 1], want_logit=True)
        o2, o3 = e.debug_head_activations(len(pairs))
        g_ov, g_lg, g_yaw = r["overlap"].cpu().numpy(), r["logit"].cpu().numpy(), r["yaw"].cpu().numpy()
        assert np.max(np.abs(g_ov - ov)) <= 1e-4, np.max(np.abs(g_ov - ov))
        assert np.all(np.abs(g_lg - lg) <= 1e-3 * (1 + np.abs(lg)))
        srt = np.sort(corr, axis=1)
        gap = (srt[:, -1] - srt[:, -2]) / np.abs(srt[:, -1])
        assert not np.any((g_yaw != yaw) & (gap > 1e-5))
        for p in range(len(pairs)):
            it = O.delta_head_forward(fv4[pairs[p, 0]][None], fv4[pairs[p, 1]][None], w, return_intermediates=True)[2]
            e2, e3 = _rel(o2[p].cpu().numpy(), it["o2"]), _rel(o3[p].cpu().numpy(), it["o3"])
            print("pair %s: c_conv2 rel err %.3g, c_conv3 rel err %.3g" % (pairs[p], e2, e3))
            assert e2 < 2e-5 and e3 < 2e-5, (pairs[p], e2, e3)
    finally:
        e.close()


# ---- 4. same bits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
def test_same_bits_across_forms_sizes_pipelines_and_calls():
    rng = np.random.default_rng(31)
    base = np.maximum(rng.normal(0.2, 1.0, size=(7, 360, 128)), 0).astype(np.float32)
    n = 4096
    e = _engine(4)
    try:
        cands = torch.from_numpy(base).cuda()[torch.arange(n) % 7].contiguous()
        query = torch.from_numpy(base[1:2]).cuda().contiguous()
        spec_l, spec_r = e.spectrum(cands), e.spectrum(query)
        dcache = e.delta_cache(cands)                       # built in the default mode: the bf16x3 mode must ignore it
        e.set_head_precision("bf16x3")
        assert not e.has_delta_cache
        full = e.heads(cands, query, want_logit=True)
        again = e.heads(cands, query, want_logit=True)
        assert torch.equal(full["logit"], again["logit"]) and torch.equal(full["yaw"], again["yaw"])
        idx = e.heads(cands, query, lidx=np.arange(n, dtype=np.int32), ridx=np.zeros(n, np.int32), want_logit=True)
        assert torch.equal(idx["logit"], full["logit"])
        for k in (1, 64, 100):
            part = e.heads(cands[:k].contiguous(), query, want_logit=True)
            assert torch.equal(part["logit"], full["logit"][:k]), k
        sp = e.heads(cands, query, spec_l=spec_l, spec_r=spec_r, want_logit=True)
        spc = e.heads(cands, query, spec_l=spec_l, spec_r=spec_r, want_logit=True, dcache_l=dcache)
        assert torch.equal(sp["logit"], full["logit"]) and torch.equal(spc["logit"], sp["logit"]) and torch.equal(spc["yaw"], sp["yaw"])
        e.set_head_pipeline(sub_chunk_pairs=256, streams=2)
        pip = e.heads(cands, query, spec_l=spec_l, spec_r=spec_r, want_logit=True)
        e.set_head_pipeline()
        assert torch.equal(pip["logit"], sp["logit"]) and torch.equal(pip["yaw"], sp["yaw"])
    finally:
        e.close()


# ---- 5. mode switching -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
def test_mode_switch_leaves_f16x3_bits_and_walk_stats_current():
    rng = np.random.default_rng(41)
    base = np.maximum(rng.normal(0.2, 1.0, size=(5, 360, 128)), 0).astype(np.float32)
    base[1][:, :40] = 0.0                     # the query has dead channels: the f16x3 sweep compacts
    e = _engine(4)
    try:
        cands = torch.from_numpy(base).cuda()[torch.arange(300) % 5].contiguous()
        query = torch.from_numpy(base[1:2]).cuda().contiguous()
        before = e.heads(cands, query, want_logit=True)
        st = e.head_walk_stats()
        assert st["compacted"] and st["live_channels"] == 88
        e.set_head_precision("bf16x3")
        mid = e.heads(cands, query, want_logit=True)
        st = e.head_walk_stats()
        assert not st["compacted"] and st["live_channels"] == 128 and st["max_slices"] == 4
        e.set_head_precision("f16x3")
        after = e.heads(cands, query, want_logit=True)
        assert torch.equal(before["logit"], after["logit"]) and torch.equal(before["yaw"], after["yaw"])
        assert not torch.equal(mid["logit"], after["logit"])
    finally:
        e.close()


# ---- 6. API ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
def test_api_engine_and_c_abi():
    e = _engine(4)
    try:
        e.set_head_precision("bf16x3")
        assert e.head_precision == "bf16x3"
        with pytest.raises(ValueError):
            e.set_head_precision("bf16x6")
        assert e.head_precision == "bf16x3"
        assert e.lib.ovn_set_head_precision(e._h, 3) == 1       # OVN_ERR_ARG
        assert e.lib.ovn_set_head_precision(e._h, -1) == 1
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")
def test_infer_precision_bf16x3(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    seq = tmp_path / "data" / "07"
    for sub in ("depth", "normal", "intensity"):
        os.makedirs(seq / sub, exist_ok=True)
    for i in range(5):
        s, shift = i % 2, 40 * (i // 2)
        for sub, key in (("depth", "range_%d"), ("normal", "normal_%d"), ("intensity", "intensity_%d")):
            np.save(seq / sub / ("%06d.npy" % i), np.roll(fixture_npz[key % s], shift, axis=1))
    cfg = {"model": dict(CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(tmp_path / "data"), "use_depth": True,
           "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False,
           "batch_size": 16, "pretrained_weightsfilename": "", "precision": "bf16x3"}
    inf = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    assert inf.engine.leg_precision == "f32" and inf.engine.head_precision == "bf16x3"
    out = [inf.infer_multiple(i, list(range(i))) for i in range(5)]
    assert inf._qa is not None and inf._qa.side.head_precision == "bf16x3" and inf._qa.side.leg_precision == "f32"
    cache = inf.feature_volumes
    assert cache.device_delta_cache is None
    feats, spec = cache.device_features, cache.device_spectra
    for i in range(1, 5):
        r = inf.engine.heads(feats, feats[i:i + 1], n=i, spec_l=spec, spec_r=spec[i:i + 1])
        assert np.array_equal(np.ravel(out[i][0]), r["overlap"].cpu().numpy()) and np.array_equal(np.ravel(out[i][1]), r["yaw"].cpu().numpy()), i
    with pytest.raises(Exception, match="bf16x3"):
        Infer(dict(cfg, precision="bf16x6"), weights=S.make_test_weights(4, seed=0))
