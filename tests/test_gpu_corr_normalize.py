"""GPU (MI355X): NormalizedCorrelation2D's normalisations (ovn_set_corr_normalization, `correlationHead_normalize`) on every route
and head precision against the fp64 restatement and its elementwise bound (tests/_corr_norm_ref.py), mode 'none' unchanged, a
known-answer test, determinism, `Infer` end to end, and DeltaLayer(negateDiffs=True) (`deltaLayer_negateDiffs`)."""
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from oracle import overlapnet_oracle as O
from tests import _corr_norm_ref as R
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

CFG = S.REFERENCE_MODEL_CFG
W4 = S.make_test_weights(4, seed=0)
PRECISIONS = ("f16x3", "f32", "bf16x3")
NORM_MODES = ("euclidean", "scaling", "standardization")


def _relu_dead(k, seed):
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, 360, 128)), 0).astype(np.float32)
    for i in range(k):
        v[i][:, rng.permutation(128)[:32]] = 0                  # a quarter of the channels dead, as under the benchmark's weights
    return v


def _sets():
    out = dict(E.value_edge_sets())
    out["relu_dead"] = _relu_dead(4, 7)
    e = np.stack([R.edge_volume(0), R.rolled(R.edge_volume(1), 29), R.edge_volume(2)])
    e[:, :, 12] = 0          # 2^100 squared is beyond fp32 in mode 'none' (the reference's own fp32 overflows there too)
    out["norm_edges"] = e
    return out


SETS = _sets()
_REF = {}


def _ref(name, i, j, mode):
    key = (name, i, j, mode)
    if key not in _REF:
        v = SETS[name]
        _REF[key] = R.corr_norm_pair(v[i], v[j], mode)
    return _REF[key]


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4)
    e.load_weights(W4, CFG)
    yield e
    e.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _routes(eng, name, prec):
    """Outputs of the four routes in the engine's current normalisation mode: pairs (i, 0) for every volume i of the set."""
    v = SETS[name]
    k = v.shape[0]
    fv = _t(v)
    query = fv[:1].contiguous()
    li = np.arange(k)
    ri = np.zeros(k, np.int64)
    out = {}
    out["corr_head"] = eng.corr_head(fv, fv, lidx=li, ridx=ri, want_corr=True)
    out["heads indexed"] = eng.heads(fv, fv, lidx=li, ridx=ri, want_logit=True, want_corr=True)
    spec, qspec = eng.spectrum(fv), eng.spectrum(query)
    out["spectral"] = eng.corr_head_spectral(spec, qspec, want_corr=True)
    dc = None
    if prec == "f16x3":
        dc = eng.delta_cache(fv)
    out["heads 1vN spectral"] = eng.heads(fv, query, spec_l=spec, spec_r=qspec, dcache_l=dc, want_logit=True, want_corr=True)
    torch.cuda.synchronize()
    return out


FORM = {"corr_head": "direct", "heads indexed": "direct", "spectral": "spectral", "heads 1vN spectral": "spectral"}


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", sorted(SETS))
def test_every_mode_route_and_precision_within_the_bound(eng, name, prec):
    k = SETS[name].shape[0]
    eng.set_head_precision(prec)
    try:
        eng.set_corr_normalization("none")
        base = _routes(eng, name, prec)
        for mode in NORM_MODES:
            eng.set_corr_normalization(mode)
            assert eng.corr_normalization == mode
            outs = _routes(eng, name, prec)
            worst = {}
            for route, r in outs.items():
                corr, yaw = r["corr"].cpu().numpy(), r["yaw"].cpu().numpy()
                for i in range(k):
                    ref = _ref(name, i, 0, mode)
                    rat = E.ratio(corr[i], ref["corr"], ref[FORM[route]])
                    worst[route] = max(worst.get(route, 0.0), rat)
                    assert rat <= 1.0, (name, prec, mode, route, i, rat)
                    assert R.yaw_ok(corr[i], 180 - int(yaw[i]), ref["corr"], ref[FORM[route]]), (name, prec, mode, route, i)
                if "overlap" in r:      # the Delta head reads the raw volumes: same bits as in mode 'none'
                    assert torch.equal(r["overlap"], base[route]["overlap"]) and torch.equal(r["logit"], base[route]["logit"])
            print("[%s %s %s] worst err / bound %s" % (name, prec, mode, {a: "%.3g" % b for a, b in worst.items()}))
    finally:
        eng.set_corr_normalization("none")
        eng.set_head_precision("f16x3")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_mode_none_is_unchanged(eng, prec):
    """'none' set explicitly, and after switching back from every other mode, gives the bits of a fresh engine on every route."""
    from overlapnet_amd.engine import OvnEngine
    fresh = OvnEngine(64, 900, 4)
    try:
        fresh.load_weights(W4, CFG)
        fresh.set_head_precision(prec)
        assert fresh.corr_normalization == "none"
        want = _routes(fresh, "relu_dead", prec)
        eng.set_head_precision(prec)
        for m in ("none",) + NORM_MODES:
            eng.set_corr_normalization(m)
            _routes(eng, "relu_dead", prec)
            eng.set_corr_normalization("none")
            got = _routes(eng, "relu_dead", prec)
            for route in want:
                for key in want[route]:
                    assert torch.equal(got[route][key], want[route][key]), (prec, m, route, key)
    finally:
        eng.set_head_precision("f16x3")
        eng.set_corr_normalization("none")
        fresh.close()


def test_mode_setter_rejects_unknown_values(eng):
    from overlapnet_amd._lib import OvnError
    with pytest.raises(ValueError):
        eng.set_corr_normalization("l2")
    assert eng.lib.ovn_set_corr_normalization(eng._h, 4) == 1 and eng.lib.ovn_set_corr_normalization(eng._h, -1) == 1
    assert eng.corr_normalization == "none"
    with pytest.raises(OvnError):
        from overlapnet_amd import _lib
        _lib.check(eng.lib.ovn_set_corr_normalization(eng._h, 7), "ovn_set_corr_normalization")


@pytest.mark.parametrize("prec", ("f16x3", "f32"))
def test_known_answer_rolled_volumes(eng, prec):
    """r = l rolled by s columns: every mode recovers yaw = 180 - bin(s) on the direct and spectral routes; under 'euclidean' the
    peak is the number of live channels (every live channel a unit vector), within the bound."""
    l = _relu_dead(1, 11)[0]
    live = int(np.count_nonzero(np.abs(l).max(axis=0)))
    shifts = (0, 1, 37, 180, 359)
    vols = np.stack([l] + [R.rolled(l, s) for s in shifts])
    fv = _t(vols)
    eng.set_head_precision(prec)
    try:
        for mode in R.MODES:
            eng.set_corr_normalization(mode)
            li = np.zeros(len(shifts), np.int64)
            ri = np.arange(1, len(shifts) + 1)
            d = eng.corr_head(fv, fv, lidx=li, ridx=ri, want_corr=True)
            spec = eng.spectrum(fv)
            sp = eng.corr_head_spectral(spec, spec, lidx=li, ridx=ri, want_corr=True)
            for p, s in enumerate(shifts):
                want_yaw = 180 - R.known_bin(s)
                for route, r in (("direct", d), ("spectral", sp)):
                    assert int(r["yaw"][p]) == want_yaw, (mode, s, route, int(r["yaw"][p]), want_yaw)
                    if mode == "euclidean":
                        ref = R.corr_norm_pair(l, vols[p + 1], mode)
                        b = R.known_bin(s)
                        assert abs(float(r["corr"][p, b]) - live) <= ref[route][b], (s, route, float(r["corr"][p, b]), live)
    finally:
        eng.set_corr_normalization("none")
        eng.set_head_precision("f16x3")


@pytest.mark.parametrize("prec", ("f16x3", "f32"))
def test_determinism_alone_in_a_sweep_and_at_another_slot(eng, prec):
    pool = _t(_relu_dead(1024, 3))
    q = pool[5:6].contiguous()
    eng.set_head_precision(prec)
    try:
        for mode in NORM_MODES:
            eng.set_corr_normalization(mode)
            spec = eng.spectrum(pool)
            one = eng.spectrum(pool[700:701].contiguous())
            assert torch.equal(spec[700], one[0]), mode
            moved = torch.roll(pool, 3, 0).contiguous()               # volume 700 at slot 703
            spec_m = eng.spectrum(moved)
            assert torch.equal(spec_m[703], spec[700]), mode
            qs = eng.spectrum(q)
            sweep = eng.heads(pool, q, spec_l=spec, spec_r=qs, want_corr=True)
            alone = eng.heads(pool[700:701].contiguous(), q, spec_l=one, spec_r=qs, want_corr=True)
            assert torch.equal(sweep["corr"][700], alone["corr"][0]) and int(sweep["yaw"][700]) == int(alone["yaw"][0])
            d_sweep = eng.corr_head(pool, q, want_corr=True)
            d_alone = eng.corr_head(pool, q, lidx=[700], ridx=[0], want_corr=True)
            d_moved = eng.corr_head(moved, q, lidx=[703], ridx=[0], want_corr=True)
            assert torch.equal(d_sweep["corr"][700], d_alone["corr"][0]) and torch.equal(d_alone["corr"][0], d_moved["corr"][0])
            torch.cuda.synchronize()
    finally:
        eng.set_corr_normalization("none")
        eng.set_head_precision("f16x3")


# ---- Infer end to end --------------------------------------------------------------------------------------------------------------

def _write_sequence(root, fx, n):
    seq = os.path.join(root, "07")
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(seq, sub), exist_ok=True)
    imgs = []
    for i in range(n):
        s, shift = i % 2, 40 * (i // 2)
        d = np.roll(fx["range_%d" % s], shift, axis=1)
        nm = np.roll(fx["normal_%d" % s], shift, axis=1)
        np.save(os.path.join(seq, "depth", "%06d.npy" % i), d)
        np.save(os.path.join(seq, "normal", "%06d.npy" % i), nm)
        imgs.append(S.stack(d, nm, None, (True, True, False)))
    return np.stack(imgs)


def _config(root, **model):
    return {"model": dict(CFG, inputShape=[64, 900], **model), "infer_seqs": "07", "data_root_folder": str(root), "use_depth": True,
            "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False,
            "batch_size": 16, "pretrained_weightsfilename": ""}


def _chain_corr(fv64, i, j, mode):
    """fp64 chain: oracle leg -> fp64 normalisation -> correlation, l = frame i, r = frame j."""
    return E.corr_pair(R.normalize64(fv64[i, 0], mode), R.normalize64(fv64[j, 0], mode))["corr"]


def _yaw_matches(yaw, refs):
    """yaw of each pair equals the fp64 chain's first maximum where its top-two gap is clear of the leg's error (1e-4 of the peak);
    elsewhere the GPU's bin must be a maximum within that."""
    for y, c in zip(np.atleast_1d(yaw), refs):
        tol = 1e-4 * np.max(np.abs(c))
        b = 180 - int(y)
        srt = np.sort(c)
        if srt[-1] - srt[-2] > 2 * tol:
            assert b == int(np.argmax(c)), (b, int(np.argmax(c)))
        else:
            assert c[b] >= srt[-1] - 2 * tol


@pytest.mark.parametrize("mode", NORM_MODES)
def test_infer_end_to_end(tmp_path, fixture_npz, mode):
    from overlapnet_amd.infer import Infer
    n = 6
    imgs = _write_sequence(tmp_path / "data", fixture_npz, n)
    w = S.make_test_weights(4, seed=0)
    fv64 = O.leg_forward(imgs, w, CFG, np.float64)
    results = {}
    for ahead in (True, False):
        cfg = dict(_config(tmp_path / "data", correlationHead_normalize=mode), stream_ahead=ahead)
        inf = Infer(cfg, weights=w)
        assert inf.engine.corr_normalization == mode
        multi, best = [], []
        for i in range(n):
            r = inf.infer_multiple(i, list(range(i)))
            if i > 0:
                _yaw_matches(r[1], [_chain_corr(fv64, j, i, mode) for j in range(i)])
                multi.append(np.atleast_1d(r[1]).copy())
        # the cached volumes' correlation vectors (direct route) against the fp64 chain
        cache = inf.feature_volumes.device_features
        c = inf.engine.corr_head(cache, cache, lidx=[0, 1, 2], ridx=[5, 5, 5], want_corr=True)["corr"].cpu().numpy()
        for p, j in enumerate((0, 1, 2)):
            ref = _chain_corr(fv64, j, 5, mode)
            assert np.max(np.abs(c[p] - ref)) <= 1e-4 * np.max(np.abs(ref)), (mode, j)
        inf.close()
        inf2 = Infer(cfg, weights=w)
        for i in range(n):
            got = inf2.infer_best_match(i, list(range(i)), overlap_thres=0.0)
            if i > 0:
                ref_id, _, yaw = got
                _yaw_matches([yaw], [_chain_corr(fv64, ref_id, i, mode)])
                best.append((ref_id, yaw))
        inf2.close()
        results[ahead] = (multi, best)
    assert all(np.array_equal(a, b) for a, b in zip(results[True][0], results[False][0]))
    assert results[True][1] == results[False][1]
    # infer_one (l = second file, r = first) and infer_multiple_vs_multiple (l = second index, r = first)
    inf = Infer(_config(tmp_path / "data", correlationHead_normalize=mode), weights=w)
    _, yaw = inf.infer_one("x/000003.bin", "y/000000.bin")
    _yaw_matches(yaw, [_chain_corr(fv64, 0, 3, mode)])
    names = ["%06d.bin" % i for i in range(n)]
    _, yaw = inf.infer_multiple_vs_multiple(names, [0, 1, 2, 5], [3, 4, 5, 1])
    _yaw_matches(yaw, [_chain_corr(fv64, j, i, mode) for i, j in zip([0, 1, 2, 5], [3, 4, 5, 1])])
    # the feature_volumes setter recomputes spectra in the mode
    vols = [fv.copy() for fv in inf.feature_volumes]
    inf.feature_volumes = vols
    spec = inf.feature_volumes.device_spectra
    feats = inf.feature_volumes.device_features
    assert torch.equal(spec, inf.engine.spectrum(feats))
    r = inf.engine.heads(feats, feats[5:6].contiguous(), spec_l=spec, spec_r=spec[5:6].contiguous())
    _yaw_matches(r["yaw"].cpu().numpy(), [_chain_corr(fv64, j, 5, mode) for j in range(len(vols))])
    inf.close()


# ---- DeltaLayer(negateDiffs=True) --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECISIONS)
def test_negate_diffs(prec):
    from overlapnet_amd.engine import OvnEngine
    sc = E.value_edge_sets()["single_column"]
    v = np.stack([sc[4], sc[0], _relu_dead(1, 5)[0]])
    fv = _t(v)
    query = fv[:1].contiguous()
    wneg = dict(W4)
    wneg["c_conv1/kernel"] = -np.asarray(W4["c_conv1/kernel"])
    a, b = OvnEngine(64, 900, 4), OvnEngine(64, 900, 4)
    try:
        a.load_weights(W4, dict(CFG, deltaLayer_negateDiffs=True))
        b.load_weights(wneg, CFG)
        assert a.negate_diffs and not b.negate_diffs
        outs = {}
        for e, tag in ((a, "a"), (b, "b")):
            dc = e.delta_cache(fv) if prec == "f16x3" else None
            e.set_head_precision(prec)
            spec, qs = e.spectrum(fv), e.spectrum(query)
            outs[tag] = [e.heads(fv, fv, lidx=[0, 1, 2], ridx=[1, 2, 0], want_logit=True),
                         e.heads(fv, query, spec_l=spec, spec_r=qs, want_logit=True),
                         e.heads(fv, query, spec_l=spec, spec_r=qs, dcache_l=dc, want_logit=True)]
        for ra, rb in zip(outs["a"], outs["b"]):
            assert torch.equal(ra["overlap"], rb["overlap"]) and torch.equal(ra["logit"], rb["logit"])
        # against the fp64 chain built on -|l - r| (DeltaLayer literal), within the head bounds
        w1 = np.asarray(W4["c_conv1/kernel"], np.float64).reshape(15, 128, 64)
        pairs = [[(0, 1), (1, 2), (2, 0)], [(0, 0), (1, 0), (2, 0)], [(0, 0), (1, 0), (2, 0)]]
        for r, pl in zip(outs["a"], pairs):
            lg, ov = r["logit"].cpu().numpy(), r["overlap"].cpu().numpy()
            for p, (i, j) in enumerate(pl):
                neg = -O.delta_layer_literal(v[i][None], v[j][None])                       # (360, 360, 128): -|l_i - r_j|
                o1 = np.asarray(W4["c_conv1/bias"], np.float64) + E._c1(neg, w1, 15)
                h = E.head_pair(v[i], v[j], W4, o1=o1)
                assert np.max(np.abs(o1 - E.head_pair(v[i], v[j], wneg)["o1"])) <= 1e-9 * np.max(np.abs(o1))
                B = E.head_bounds(h, W4, prec)
                assert E.ratio(lg[p], h["logit"], B["logit"]) <= 1 and E.ratio(ov[p], h["overlap"], B["overlap"]) <= 1, (prec, i, j)
    finally:
        a.close()
        b.close()
