"""GPU (MI355X): every stage of the Delta head and the leg against ELEMENTWISE error bounds derived from the arithmetic
(oracle/error_bounds.py), on volumes at the value edges of the fast paths, across the head routes and modes, and on every leg
input shape the C ABI accepts at the edges of its range.  Each test prints its worst err / bound per stage (<= 1 passes)."""
import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from tools import synthetic as S
from overlapnet_amd import weights as WT
from overlapnet_amd._lib import OvnError

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

CFG = S.REFERENCE_MODEL_CFG
W4 = S.make_test_weights(4, seed=0)
SETS = E.value_edge_sets()
_ORACLE = {}


def _oracle(name, i, j, w=W4, s=15):
    key = (name, i, j, s)
    if key not in _ORACLE:
        v = SETS[name]
        _ORACLE[key] = (E.head_pair(v[i], v[j], w, s), E.corr_pair(v[i], v[j]))
    return _ORACLE[key]


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4)
    e.load_weights(W4, CFG)
    yield e
    e.close()


def _check(tag, r, pairs, name, mode, o2=None, o3=None, corr_form="direct", w=W4, s=15):
    worst = {}
    lg, ov = r["logit"].cpu().numpy(), r["overlap"].cpu().numpy()
    g_corr = r["corr"].cpu().numpy() if "corr" in r else None
    for p, (i, j) in enumerate(pairs):
        h, c = _oracle(name, i, j, w, s)
        B = E.head_bounds(h, w, mode)
        rat = {"logit": E.ratio(lg[p], h["logit"], B["logit"]), "overlap": E.ratio(ov[p], h["overlap"], B["overlap"])}
        if g_corr is not None:
            rat["corr"] = E.ratio(g_corr[p], c["corr"], c[corr_form])
        if o2 is not None and p < o2.shape[0]:
            rat["o2"] = E.ratio(o2[p], h["o2"], B["o2"])
            rat["o3"] = E.ratio(o3[p], h["o3"], B["o3"])
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("[%s %s %s] worst err / bound: %s" % (name, mode, tag, {k: "%.3g" % v for k, v in sorted(worst.items())}))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, "[%s %s %s] over the bound: %s" % (name, mode, tag, bad)
    return worst


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3", "f32"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_head_value_edges_routes_and_modes(eng, name, mode):
    v = SETS[name]
    k = v.shape[0]
    fv = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    cands, query = fv, fv[:1].contiguous()
    eng.set_head_precision("f16x3")
    cache = eng.delta_cache(cands)
    eng.set_head_precision(mode)
    try:
        spec, qspec = eng.spectrum(cands), eng.spectrum(query)
        # indexed pairs (both roles of the query), direct correlation; o2 / o3 of every pair
        pairs = [(i, 0) for i in range(k)] + [(0, 1)]
        if name == "subnormal":
            # two volumes of subnormals: every product of the correlation is below fp32's smallest subnormal, so the fp32 result
            # is 0 (the bound's subnormal floor), and the Delta head's pair scale stays clamped at 2^100 (the bound's f16x3 floor)
            pairs.append((1, 1))
        li, ri = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        r = eng.heads(fv, fv, lidx=li, ridx=ri, want_logit=True, want_corr=True)
        o2, o3 = [t.cpu().numpy() for t in eng.debug_head_activations(len(pairs))]
        _check("indexed", r, pairs, name, mode, o2, o3)
        ind = r
        sweep = [(i, 0) for i in range(k)]
        outs = {}
        for route, comp, dc in (("1vN scratch", True, None), ("1vN cache+compaction", True, cache), ("1vN cache, no compaction", False, cache)):
            if dc is not None and mode != "f16x3":
                dc = None                     # the Delta cache rows exist for the f16x3 mode only
            eng.set_head_compaction(comp)
            try:
                r = eng.heads(cands, query, spec_l=spec, spec_r=qspec, dcache_l=dc, want_logit=True, want_corr=True)
                o2, o3 = [t.cpu().numpy() for t in eng.debug_head_activations(k)]
            finally:
                eng.set_head_compaction(True)
            _check(route + " spectral", r, sweep, name, mode, o2, o3, corr_form="spectral")
            outs[route] = r
        r = eng.heads(cands, query, want_logit=True, want_corr=True)          # 1-vs-N with the direct correlation
        _check("1vN direct", r, sweep, name, mode)
        outs["1vN direct"] = r
    finally:
        eng.set_head_precision("f16x3")
    # bits the code promises to be equal: cache rows or scratch; yaw of every route = the oracle's except at its near-ties
    a, b = outs["1vN scratch"], outs["1vN cache+compaction"]
    assert torch.equal(a["logit"], b["logit"]) and torch.equal(a["yaw"], b["yaw"])
    for route, r in list(outs.items()) + [("indexed", ind)]:
        n = k
        corr = np.stack([_oracle(name, i, 0)[1]["corr"] for i in range(n)])
        srt = np.sort(corr, axis=1)
        with np.errstate(all="ignore"):
            gap = np.nan_to_num((srt[:, -1] - srt[:, -2]) / np.abs(srt[:, -1]))
        yaw = 180 - np.argmax(corr, axis=1)
        g = r["yaw"].cpu().numpy()[:n]
        assert not np.any((g != yaw) & (gap > 1e-5)), (route, g, yaw, gap)


def _want_packed_steps(live):
    """MFMA steps of the packed last slice (ovn_head_walk_stats): 0 when the last slice holds more than 16 live channels."""
    n_last = live - 32 * ((live + 31) // 32 - 1)
    return 0 if n_last > 16 else 3 * (-(-(-(-15 // (32 // n_last))) // 3))


QUERY_CASES = [("single_column", q) for q in range(4)] + [("pow2_edge", q) for q in range(3)]


@pytest.mark.parametrize("name,q", QUERY_CASES)
def test_query_dependent_paths_of_the_sweep(eng, name, q):
    """What depends on the QUERY of a 1-vs-N sweep (f16x3, the mode with Delta cache rows and compaction): its live channels
    (97 / 111 / 112 / 113 -> packed last slices of 1 / 15 / 16 channels, and 17, which is not packed) and its largest value
    (exactly 4, one ulp below, one ulp above: the query's own scale bucket against candidates on both sides of it, so both
    sides of the cache-row validity rule).  Every sweep against the bound, with and without cache rows (same bits) and with
    compaction off."""
    v = SETS[name]
    k = v.shape[0]
    fv = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    query = fv[q:q + 1].contiguous()
    sweep = [(i, q) for i in range(k)]
    assert eng.head_precision == "f16x3"
    spec, qspec, cache = eng.spectrum(fv), eng.spectrum(query), eng.delta_cache(fv)
    live = int(np.count_nonzero((v[q] != 0).any(axis=0)))
    res = {}
    for route, comp, dc in (("cache+compaction", True, cache), ("scratch+compaction", True, None), ("no compaction", False, cache)):
        eng.set_head_compaction(comp)
        try:
            r = eng.heads(fv, query, spec_l=spec, spec_r=qspec, dcache_l=dc, want_logit=True, want_corr=True)
            st = eng.head_walk_stats()
            o2, o3 = [t.cpu().numpy() for t in eng.debug_head_activations(k)]
        finally:
            eng.set_head_compaction(True)
        if comp and live < 128:
            assert st["compacted"] and st["live_channels"] == live, (route, st)
            assert st["packed_last_slice_steps"] == _want_packed_steps(live), (route, live, st)
        if not comp:
            assert not st["compacted"]
        _check("query %d %s" % (q, route), r, sweep, name, "f16x3", o2, o3, corr_form="spectral")
        res[route] = r
    if name == "single_column":
        assert [_want_packed_steps(n) > 0 for n in (97, 111, 112, 113)] == [True, True, True, False]
    a, b = res["cache+compaction"], res["scratch+compaction"]
    assert torch.equal(a["logit"], b["logit"]) and torch.equal(a["yaw"], b["yaw"])


@pytest.mark.parametrize("s", [10, 24])
def test_generic_conv1size_against_the_bound(s):
    """conv1NetworkHead_conv1size 10 / 24: the generic fp32 path in its own arithmetic (|l - r| formed exactly).  It keeps no
    c_conv2 / c_conv3 activations for the test hook (ovn_debug_head_activations: OVN_ERR_STATE), so logit, overlap and corr only."""
    from overlapnet_amd.engine import OvnEngine
    cfg = dict(CFG, conv1NetworkHead_conv1size=s)
    w = S.make_test_weights(4, seed=3, model_cfg=cfg)
    e = OvnEngine(64, 900, 4)
    try:
        e.load_weights(w, cfg)
        for name in ("neg_zero", "tiny_negative", "wide_range"):
            v = SETS[name]
            fv = torch.from_numpy(np.ascontiguousarray(v)).cuda()
            pairs = [(i, 0) for i in range(v.shape[0])] + [(0, 1)]
            r = e.heads(fv, fv, lidx=[p[0] for p in pairs], ridx=[p[1] for p in pairs], want_logit=True, want_corr=True)
            _check("generic s=%d" % s, r, pairs, name, "generic", w=w, s=s)
            with pytest.raises(OvnError, match="call right after ovn_heads"):
                e.debug_head_activations(1)
    finally:
        e.close()


LEG_SHAPES = [(h, w) for h in (49, 50, 63, 65, 79, 80) for w in (899, 900)]
LAYER_SHAPES = [(49, 899), (65, 900)]     # every layer in isolation as well (ovn_debug_conv) at these


def _leg_layers_in_isolation(h, w, C, imgs, wts, chain):
    """Each leg layer alone (ovn_debug_conv: the per-layer conv kernels of conv_f32.hip / conv_f16x3.hip), on the fp32 rounding of
    its exact input, against that layer's own bound, in both leg modes."""
    from overlapnet_amd import _lib
    from overlapnet_amd.engine import OvnEngine, _ptr
    x = imgs
    for l, (name, ref_out, _) in zip(WT.leg_layers(C, CFG), chain):
        assert l.name == name
        eng = OvnEngine(h, w, l.cin)
        try:
            kt = torch.from_numpy(wts[name + "/kernel"]).cuda()
            bt = torch.from_numpy(wts[name + "/bias"]).cuda()
            st = eng._stream()
            _lib.check(eng.lib.ovn_add_leg_layer(eng._h, name.encode(), _ptr(kt), _ptr(bt), l.kh, l.kw, l.cin, l.cout, l.sh, l.sw, st),
                       "ovn_add_leg_layer")
            oh, ow = (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1
            xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            out = torch.empty((x.shape[0], oh, ow, l.cout), dtype=torch.float32, device="cuda")
            ref, B = E.leg_layer_bound(x, wts[name + "/kernel"], wts[name + "/bias"], (l.sh, l.sw))
            for mode in ("f16x3", "f32"):
                eng.set_leg_precision(mode)
                out.fill_(float("nan"))
                _lib.check(eng.lib.ovn_debug_conv(eng._h, 0, _ptr(xt), x.shape[0], h, w, _ptr(out), st), "ovn_debug_conv")
                torch.cuda.synchronize()
                rt = E.ratio(out.cpu().numpy(), ref, B[mode])
                print("[leg layer %s %dx%d C=%d %s] worst err / bound: %.3g" % (name, h, w, C, mode, rt))
                assert rt <= 1.0, (name, h, w, C, mode, rt)
        finally:
            eng.close()
        x = ref_out.astype(np.float32)
        h, w = oh, ow


def _leg_case(h, w, C, seed):
    """The whole leg (its fast kernels, chosen by layer shape) at input h x w x C, both modes, against the bound of its output;
    the fp64 leg is computed once for both modes."""
    from overlapnet_amd.engine import OvnEngine
    rng = np.random.default_rng(seed)
    imgs = rng.normal(0.5, 1.0, size=(2, h, w, C)).astype(np.float32)
    wts = S.make_test_weights(C, seed=0)
    bounds = E.leg_with_bounds(imgs, wts, ("f16x3", "f32"), CFG)
    e = OvnEngine(h, w, C)
    try:
        e.load_weights(wts, CFG)
        for mode in ("f16x3", "f32"):
            e.set_leg_precision(mode)
            out = e.leg(torch.from_numpy(imgs).cuda()).cpu().numpy()
            name, x, B = bounds[mode][-1]
            rt = E.ratio(out, x.reshape(out.shape), B.reshape(out.shape))
            print("[leg %dx%d C=%d %s] worst err / bound of %s: %.3g" % (h, w, C, mode, name, rt))
            assert rt <= 1.0, (h, w, C, mode, rt)
        e.set_leg_precision("f16x3")
    except Exception:
        e.close()
        raise
    if (h, w) in LAYER_SHAPES:
        try:
            _leg_layers_in_isolation(h, w, C, imgs, wts, bounds["f32"])
        except Exception:
            e.close()
            raise
    return e, imgs


@pytest.mark.parametrize("h,w", LEG_SHAPES)
def test_leg_shapes_against_the_bound(h, w):
    assert WT.leg_output_shape(h, w, WT.leg_layers(4, CFG)) == (1, 360, 128)
    e, imgs = _leg_case(h, w, 4, seed=h * 1000 + w)
    try:
        if (h, w) == (63, 899):           # batch independence at an odd shape: a scan alone or in a batch, the same bits
            a = torch.from_numpy(imgs).cuda()
            one = e.leg(a[1:2].contiguous())
            many = e.leg(torch.cat([a, (300 * a[:1]).contiguous(), a[1:2]]).contiguous())
            assert torch.equal(many[1:2], one) and torch.equal(many[3:4], one)
    finally:
        e.close()


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("h,w", LAYER_SHAPES)
def test_leg_generic_first_layer_shapes(h, w, C):
    e, _ = _leg_case(h, w, C, seed=C * 7 + h)
    e.close()
