"""GPU (MI355X): feature widths other than 360 -- the leg, both heads (delta_head.hip, corr_head.hip, delta_head_generic.hip at a
runtime W), launch-shape independence and `Infer` end to end, against the fp64 oracle.  Tolerances of tests/test_gpu_parity.py:
overlap |d| <= 1e-4, logit <= 1e-3 (1 + |logit|), corr / activations <= 2e-5 max|oracle|, identical yaw bin unless the oracle's
top-two gap is below 1e-5 relative."""
import os

import numpy as np
import pytest
import torch

from oracle import overlapnet_oracle as O
from tests import _corr_norm_ref as R
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

A3 = {"additional_unsymmetric_layer3a": True}
# feature width -> (input H, W, model keys) of a leg that produces it
GEOM = {270: (64, 720, A3), 371: (32, 900, {}), 422: (64, 1024, A3), 433: (32, 1024, {})}
PRECISIONS = ("f32", "f16x3", "bf16x3")


def _cfg(fw, **extra):
    h, w, keys = GEOM[fw]
    return dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=fw,
                additional_unsymmetric_layer3a=bool(keys.get("additional_unsymmetric_layer3a", False)), **extra)


def _weights(fw, seed=0, **extra):
    return S.make_test_weights(4, seed=seed, model_cfg=_cfg(fw, **extra), feat_w=fw)


def _engine(fw, w, **extra):
    from overlapnet_amd.engine import OvnEngine
    h, wi, _ = GEOM[fw]
    e = OvnEngine(h, wi, 4)
    e.load_weights(w, _cfg(fw, **extra))
    assert e.feat_w == fw
    return e


def _volumes(fw, k, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, fw, 128)), 0).astype(np.float32) * np.float32(scale)
    for i in range(k):
        v[i][:, rng.permutation(128)[:32]] = 0
    return v


def _yaw_ok(g_yaw, o_yaw, corr):
    for i in range(len(o_yaw)):
        if g_yaw[i] == o_yaw[i]:
            continue
        top = np.sort(corr[i])[::-1]
        assert (top[0] - top[1]) <= 1e-5 * abs(top[0]), "yaw bin %d vs oracle %d with a clear top-two gap" % (g_yaw[i], o_yaw[i])


def _check_heads(out, fl, fr, w, conv1size=15, ref=None):
    ov, yaw, lg, corr = ref if ref is not None else O.heads_forward(fl[:, None], fr[:, None], w, conv1size)
    g_ov = out["overlap"].cpu().numpy()
    g_lg = out["logit"].cpu().numpy()
    g_corr = out["corr"].cpu().numpy()
    assert np.max(np.abs(g_ov - ov)) <= 1e-4
    assert np.all(np.abs(g_lg - lg) <= 1e-3 * (1 + np.abs(lg))), (g_lg, lg)
    assert g_corr.shape == corr.shape
    assert np.max(np.abs(g_corr - corr)) <= 2e-5 * np.max(np.abs(corr))
    _yaw_ok(out["yaw"].cpu().numpy(), yaw, corr)


# ---- 2. the leg ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fw", [371, 422])
@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_leg_other_widths(fw, prec, fixture_npz):
    h, wi, _ = GEOM[fw]
    imgs = []
    for i in range(2):
        x = S.stack(fixture_npz["range_%d" % i], fixture_npz["normal_%d" % i], None, (True, True, False))   # (64, 900, 4)
        x = x[::64 // h] if h < 64 else x
        x = np.concatenate([x, x[:, :wi - x.shape[1]]], axis=1) if wi > x.shape[1] else x[:, :wi]
        imgs.append(np.ascontiguousarray(x, np.float32))
    imgs = np.stack(imgs)
    w = _weights(fw)
    e = _engine(fw, w)
    try:
        e.set_leg_precision(prec)
        fv = e.leg(torch.from_numpy(imgs).cuda()).cpu().numpy()
    finally:
        e.close()
    ref = O.leg_forward(imgs, w, _cfg(fw))[:, 0]
    assert fv.shape == ref.shape == (2, fw, 128)
    assert np.max(np.abs(fv - ref)) <= 2e-5 * np.max(np.abs(ref))


# ---- 3. the heads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fw", [270, 371, 422, 433])
def test_heads_other_widths_every_precision(fw):
    w = _weights(fw)
    e = _engine(fw, w)
    try:
        sets = {"relu": _volumes(fw, 3, 1), "large": _volumes(fw, 3, 2, scale=300.0)}
        li, ri = [0, 1, 2, 2], [1, 2, 0, 2]
        refs = {name: O.heads_forward(v[li][:, None], v[ri][:, None], w) for name, v in sets.items()}
        for prec in PRECISIONS:
            e.set_head_precision(prec)
            for name, v in sets.items():
                ft = torch.from_numpy(v).cuda()
                out = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True, want_corr=True)
                _check_heads(out, v[li], v[ri], w, ref=refs[name])
                c = e.corr_head(ft, ft, lidx=li, ridx=ri, want_corr=True)
                assert torch.equal(c["corr"], out["corr"]) and torch.equal(c["yaw"], out["yaw"])
    finally:
        e.close()


def test_heads_normalize_negate_conv1size():
    fw = 371
    v = _volumes(fw, 3, 5)
    li, ri = [0, 1, 2], [1, 2, 0]
    delta_ref = {}
    for mode in ("none", "euclidean", "scaling", "standardization"):
        for negate in (False, True):
            w = _weights(fw, seed=3)
            e = _engine(fw, w, correlationHead_normalize=mode, deltaLayer_negateDiffs=negate)
            try:
                e.set_head_precision("f32")
                ft = torch.from_numpy(v).cuda()
                out = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True, want_corr=True)
            finally:
                e.close()
            wr = dict(w)
            if negate:      # DeltaLayer(negateDiffs=True): -|l - r| through a linear c_conv1 = |l - r| through the negated kernel
                wr["c_conv1/kernel"] = -w["c_conv1/kernel"]
            ln, rn = R.normalize64(v[li], mode), R.normalize64(v[ri], mode)
            corr = O.correlation_head_forward(ln[:, None], rn[:, None])
            if negate not in delta_ref:
                delta_ref[negate] = O.delta_head_forward(v[li][:, None], v[ri][:, None], wr)
            ov, lg = delta_ref[negate]
            _check_heads(out, v[li], v[ri], wr, ref=(ov, O.yaw_from_orientation(corr), lg, corr))
    # conv1NetworkHead_conv1size = 10: G = 37 groups, the general fp32 path at W = 371
    w = _weights(fw, seed=4, conv1NetworkHead_conv1size=10)
    assert w["overlap_output/kernel"].shape == (35 * 35 * 256, 1)
    e = _engine(fw, w, conv1NetworkHead_conv1size=10)
    try:
        ft = torch.from_numpy(v).cuda()
        out = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True, want_corr=True)
    finally:
        e.close()
    _check_heads(out, v[li], v[ri], w, conv1size=10)


# ---- 4. the same bits for every launch shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fw", [371, 433])
def test_same_bits_across_launch_shapes(fw):
    w = _weights(fw)
    e = _engine(fw, w)
    try:
        v = torch.from_numpy(_volumes(fw, 9, 7)).cuda()
        q = v[4:5]
        for prec in ("f32", "f16x3"):
            e.set_head_precision(prec)
            e.set_head_pipeline(1024)
            a = e.heads(v, q, want_logit=True, want_corr=True)                          # 1-vs-N
            b = e.heads(v, v, lidx=list(range(9)), ridx=[4] * 9, want_logit=True, want_corr=True)   # the same pairs by index
            parts = [e.heads(v[i:i + 2], q, want_logit=True, want_corr=True) for i in range(0, 9, 2)]   # small sweeps
            for k in ("overlap", "logit", "yaw", "corr"):
                assert torch.equal(a[k], b[k]), k
                assert torch.equal(a[k], torch.cat([p[k] for p in parts])), k
            for chunk in (1, 4):
                e.set_head_pipeline(chunk)
                c = e.heads(v, q, want_logit=True, want_corr=True)
                for k in ("overlap", "logit", "yaw", "corr"):
                    assert torch.equal(a[k], c[k]), (k, chunk)
            e.set_head_pipeline(1024)
    finally:
        e.close()


def test_width_371_delta_head_matches_360_fp32(capsys):
    """At W = 371, G = 24: the Delta head reads only columns < 360 of both volumes, and both engines launch delta_c12_kernel<3, 2>,
    c_conv3 and dense_sigmoid_kernel over (24 - 2)^2 * 256 inputs on the same operands: overlap and logit have the bits of the 360
    fp32 mode's on feats[:, :360]."""
    w371 = _weights(371)
    e371 = _engine(371, w371)
    from overlapnet_amd.engine import OvnEngine
    e360 = OvnEngine(64, 900, 4)
    try:
        w360 = S.make_test_weights(4, seed=0)
        for k in ("c_conv1", "c_conv2", "c_conv3", "overlap_output"):      # the same head weights in both engines
            for p in ("kernel", "bias"):
                w360[k + "/" + p] = w371[k + "/" + p]
        e360.load_weights(w360, S.REFERENCE_MODEL_CFG)
        e360.set_head_precision("f32")
        e371.set_head_precision("f32")
        v = _volumes(371, 6, 11)
        v371 = torch.from_numpy(v).cuda()
        v360 = torch.from_numpy(np.ascontiguousarray(v[:, :360])).cuda()
        li, ri = [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0]
        a = e371.heads(v371, v371, lidx=li, ridx=ri, want_logit=True)
        b = e360.heads(v360, v360, lidx=li, ridx=ri, want_logit=True)
        d = float(torch.max(torch.abs(a["overlap"] - b["overlap"])))
        with capsys.disabled():
            print("\nW=371 vs 360 fp32 Delta head: max |d overlap| = %.3g" % d)
        assert torch.equal(a["overlap"], b["overlap"]) and torch.equal(a["logit"], b["logit"])
    finally:
        e371.close()
        e360.close()


def test_360_only_entry_points_raise_at_other_widths():
    from overlapnet_amd._lib import OvnError
    e = _engine(371, _weights(371))
    try:
        v = torch.from_numpy(_volumes(371, 2, 3)).cuda()
        assert not e.has_delta_cache and not e.has_spectrum
        with pytest.raises(OvnError):
            e.spectrum(v)
        with pytest.raises(OvnError):
            e.delta_cache(v)
        spec = torch.zeros((2, 128, e.SPEC_W), device=v.device)
        with pytest.raises(OvnError):
            e.corr_head_spectral(spec, spec[:1])
        with pytest.raises(OvnError):
            e.heads(v, v[:1], spec_l=spec, spec_r=spec[:1])
        with pytest.raises(OvnError):       # volumes of the wrong width
            e.heads(torch.zeros((2, 360, 128), device=v.device), v[:1])
    finally:
        e.close()


# ---- 5. Infer end to end at 32 x 900 -------------------------------------------------------------------------------------------
def _write_cues(root, fx, n):
    seq = os.path.join(root, "07")
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(seq, sub), exist_ok=True)
    imgs = []
    for i in range(n):
        s, shift = i % 2, 40 * (i // 2)
        d = np.ascontiguousarray(np.roll(fx["range_%d" % s], shift, axis=1)[::2])       # a 32-beam image: every second row
        nm = np.ascontiguousarray(np.roll(fx["normal_%d" % s], shift, axis=1)[::2])
        np.save(os.path.join(seq, "depth", "%06d.npy" % i), d)
        np.save(os.path.join(seq, "normal", "%06d.npy" % i), nm)
        imgs.append(S.stack(d, nm, None, (True, True, False)))
    return np.stack(imgs)


def _infer_cfg(root, **extra):
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[32, 900], leg_output_width=371, additional_unsymmetric_layer3a=False),
           "infer_seqs": "07", "data_root_folder": str(root), "use_depth": True, "use_normals": True, "use_class_probabilities": False,
           "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


def test_infer_end_to_end_32x900(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd._lib import OvnError
    n = 5
    imgs = _write_cues(str(tmp_path / "data"), fixture_npz, n)
    mcfg = _infer_cfg(tmp_path / "data")["model"]
    w = S.make_test_weights(4, seed=0, model_cfg=mcfg, feat_w=371)
    pairs = np.array([[i, j] for i in range(n) for j in range(n)])
    ov, yaw, lg, corr, fv = O.infer_pairs(imgs, pairs, w, mcfg)
    ov = ov.reshape(n, n)
    yaw = yaw.reshape(n, n)
    corr = corr.reshape(n, n, 371)
    results = {}
    for ahead in (True, False):
        inf = Infer(_infer_cfg(tmp_path / "data", stream_ahead=ahead, precision="f32"), weights=w)
        try:
            assert inf.feat_w == 371
            got_fv = inf.create_feature_volumes(["%06d" % i for i in range(n)])
            assert got_fv.shape == (n, 1, 371, 128)
            assert np.max(np.abs(got_fv - fv)) <= 2e-5 * np.max(np.abs(fv))
            o1, y1 = inf.infer_one(str(tmp_path / "000001.bin"), str(tmp_path / "000000.bin"))
            # infer_one(f1, f2): pair (f2 -> l, f1 -> r) as in the reference's file order
            assert abs(float(np.asarray(o1).reshape(-1)[0]) - ov[0, 1]) <= 1e-4
            assert inf.infer_multiple(0, []) is None
            seq = []
            for i in range(1, n):
                o, y = inf.infer_multiple(i, list(range(i)))
                o, y = np.atleast_1d(o).copy(), np.atleast_1d(y).copy()
                seq.append((o, y))
                for j in range(i):
                    assert abs(float(o[j]) - ov[j, i]) <= 1e-4
                    if y[j] != yaw[j, i]:
                        _yaw_ok([y[j]], [yaw[j, i]], corr[j, i][None])
            assert len(inf.feature_volumes) == n and inf.feature_volumes.shape == (n, 1, 371, 128)
            b = inf.infer_best_match(n - 1, list(range(n - 1)), 0.0)
            m = inf.infer_multiple_vs_multiple(["%06d" % i for i in range(n)], [0, 1, 2], [3, 4, 4])
            inf.feature_volumes = [fv[i] for i in range(n)]
            o2, y2 = inf.infer_multiple(0, [1, 2, 3])
            with pytest.raises(OvnError):
                inf.engine.spectrum(torch.from_numpy(fv[:1, 0]).cuda())
            results[ahead] = (o1, y1, seq, b, m, o2, y2)
        finally:
            inf.close()
        o_m = np.asarray(m[0]).reshape(-1)
        for k, (i, j) in enumerate([(3, 0), (4, 1), (4, 2)]):     # second -> head-left, first -> head-right
            assert abs(float(o_m[k]) - ov[i, j]) <= 1e-4
        for k, j in enumerate([1, 2, 3]):
            assert abs(float(np.asarray(o2).reshape(-1)[k]) - ov[j, 0]) <= 1e-4
    a, b = results[True], results[False]
    assert np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
    for (oa, ya), (ob, yb) in zip(a[2], b[2]):
        assert np.array_equal(oa, ob) and np.array_equal(ya, yb)
    assert repr(a[3]) == repr(b[3])
