"""GPU (MI355X): the scratch every entry point reserves, pinned, with the result the suite already asserts for that route.

Every consumer of the context's scratch block sizes and places its buffers through ONE layout struct (csrc/ovn_scratch.h).  Each case
here makes ONE call on a fresh engine and reads `workspace_bytes()`: on a fresh context that is need + need // 8, so it pins the
reserved total exactly.  PARENT holds the values the same cases gave before the layouts existed (commit d489cf9, hand-written sums,
MI355X; profiles/scratch_layout.json has both sides): the layouts of the default head (f16x3 / bf16x3 at 360 columns, segmented passes
included) must reserve exactly that; the fp32, generic, training, leg and projection routes carried hand-added slop and may reserve
less, never more.  Then the case checks the call's result the way the suite checks that route elsewhere: bit-equality with the
unchunked / per-query form, or the route's fp64 bound.  Shapes are the smallest that reach each layout variant."""
import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from oracle import overlapnet_oracle as O
from overlapnet_amd import weights as WT
from tests import _feature_grad_ref as F
from tests import _head_grad_ref as R
from tests import _leg_geometry_ref as G
from tests import _leg_grad_ref as L
from tests import _split_width_ref as SR
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

CFG = S.REFERENCE_MODEL_CFG
A2_IN_YAW_MAX_PAIRS = 64      # OVN_A2_IN_YAW_MAX_PAIRS (csrc/ovn_internal.h)

# case -> (workspace_bytes() at the parent commit d489cf9 on the MI355X, must the new value EQUAL it?)
PARENT = {
    "sweep3_dcache": (12070080, True),
    "sweep65": (214351200, True),
    "indexed3": (12180672, True),
    "pipeline20": (35878176, True),
    "bf16x3": (13853088, True),
    "f32": (2669238, False),
    "width_split45": (20214, False),
    "generic_s10": (132480, False),
    "segments_compact": (32295744, True),
    "segments_plain": (25452000, True),
    "delta_head_grad": (7207200, False),
    "heads_feature_grad": (21378528, False),
    "leg": (1914048, False),
    "leg_backward": (11499840, False),
    "debug_conv_grad": (4254336, False),
    "project_idx": (1046304, False),
}


def _ws(e, case):
    """workspace_bytes() after the case's one call (printed: the record of profiles/scratch_layout.json)."""
    b = e.workspace_bytes()
    print("SCRATCH %s %d" % (case, b))
    return b


def _pin(case, got):
    want, exact = PARENT[case]
    assert got % 9 == 0, "a fresh context reserves need + need // 8 with need a multiple of 256"
    assert (got == want) if exact else (0 < got <= want), "%s: reserves %d bytes, the parent %d" % (case, got, want)


def _engine(h=64, w=900, c=4, weights=None, cfg=CFG):
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(h, w, c)
    try:
        e.load_weights(S.make_test_weights(4, seed=0) if weights is None else weights, cfg)
        assert e.workspace_bytes() == 0
    except Exception:
        e.close()
        raise
    return e


# ---- the default geometry: four volumes, the pairs (0, 3), (1, 3), (2, 3) and their fp64 oracle, computed once ---------------------
@pytest.fixture(scope="module")
def vols():
    rng = np.random.default_rng(46)
    v = np.maximum(rng.normal(0.3, 1.0, size=(4, 360, 128)), 0).astype(np.float32)   # asymmetric: a swapped role cannot pass
    v[1][:, rng.permutation(128)[:32]] = 0
    w = S.make_test_weights(4, seed=0)
    l, r = v[[0, 1, 2]][:, None].astype(np.float64), v[[3, 3, 3]][:, None].astype(np.float64)
    inters = [O.delta_head_forward(l[p:p + 1], r[p:p + 1], w, return_intermediates=True) for p in range(3)]
    corr = O.correlation_head_forward(l, r)
    return {"v": v, "ov": np.concatenate([np.reshape(i[0], -1) for i in inters]), "lg": np.concatenate([np.reshape(i[1], -1) for i in inters]),
            "o2": [i[2]["o2"] for i in inters], "o3": [i[2]["o3"] for i in inters], "corr": corr, "yaw": O.yaw_from_orientation(corr)}


def _check_first3(out, vols):
    """The three pairs against the fp64 oracle with the gates of tests/test_gpu_parity.py."""
    g_ov, g_lg, g_yaw = (out[k][:3].cpu().numpy() for k in ("overlap", "logit", "yaw"))
    assert np.max(np.abs(g_ov - vols["ov"])) <= 1e-4
    assert np.all(np.abs(g_lg - vols["lg"]) <= 1e-3 * (1 + np.abs(vols["lg"])))
    srt = np.sort(vols["corr"], axis=1)
    gap = (srt[:, -1] - srt[:, -2]) / np.abs(srt[:, -1])
    assert not np.any((g_yaw != vols["yaw"]) & (gap > 1e-5))


def _same(a, b, what):
    for k in ("overlap", "yaw", "logit"):
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("n,case", [(3, "sweep3_dcache"), (A2_IN_YAW_MAX_PAIRS + 1, "sweep65")])
def test_spectral_sweep(vols, n, case):
    """1-vs-n spectral sweep: up to 64 pairs the yaw launch fills the sub-chunk's a2raw (and here the candidates carry Delta cache
    rows), one pair more and the Delta head computes it.  == the indexed form of the same pairs, bit for bit."""
    e = _engine()
    try:
        pool = torch.from_numpy(vols["v"]).cuda()
        cands = pool[torch.arange(n) % 3].contiguous()
        query = pool[3:4].contiguous()
        spec_c, spec_q = e.spectrum(cands), e.spectrum(query)
        dc = e.delta_cache(cands) if n == 3 else None
        assert e.workspace_bytes() == 0
        out = e.heads(cands, query, want_logit=True, spec_l=spec_c, spec_r=spec_q, dcache_l=dc)
        ws = _ws(e, case)
        assert e.head_walk_stats()["compacted"]
        allf, alls = torch.cat([cands, query]), torch.cat([spec_c, spec_q])       # the query BEHIND the candidates: same slots
        idx = e.heads(allf, allf, lidx=np.arange(n), ridx=np.full(n, n), want_logit=True, spec_l=alls, spec_r=alls)
        _same(out, idx, "1-vs-n against indexed")
        _check_first3(out, vols)
    finally:
        e.close()
    _pin(case, ws)


def test_indexed_pairs(vols):
    """3 indexed pairs: per-pair right volumes (a2raw for each)."""
    e = _engine()
    try:
        pool = torch.from_numpy(vols["v"]).cuda()
        out = e.heads(pool, pool, lidx=[0, 1, 2], ridx=[3, 3, 3], want_logit=True)
        ws = _ws(e, "indexed3")
        _check_first3(out, vols)
    finally:
        e.close()
    _pin("indexed3", ws)


def test_pipeline_sub_chunks(vols):
    """20 pairs in chunks of 8, sub-chunks of 3 on two streams: three sub-chunk blocks (3 + 3 + 2 pairs), a short last chunk of 4 =
    3 + 1.  == the default pipeline, bit for bit."""
    e = _engine()
    try:
        pool = torch.from_numpy(vols["v"]).cuda()
        cands = pool[torch.arange(20) % 3].contiguous()
        query = pool[3:4].contiguous()
        e.set_head_pipeline(chunk_pairs=8, sub_chunk_pairs=3, streams=2)
        out = e.heads(cands, query, want_logit=True)
        ws = _ws(e, "pipeline20")
        e.set_head_pipeline()
        _same(out, e.heads(cands, query, want_logit=True), "pipeline against default")
        _check_first3(out, vols)
    finally:
        e.close()
    _pin("pipeline20", ws)


def test_bf16x3_head(vols):
    e = _engine()
    try:
        pool = torch.from_numpy(vols["v"]).cuda()
        e.set_head_precision("bf16x3")
        out = e.heads(pool, pool, lidx=[0, 1, 2], ridx=[3, 3, 3], want_logit=True)
        ws = _ws(e, "bf16x3")
        _check_first3(out, vols)
    finally:
        e.close()
    _pin("bf16x3", ws)


def test_f32_head_and_its_debug_hooks(vols):
    """The fp32 route on 3 pairs; o2 and o3 read back through the hooks the call left, against the oracle's activations."""
    e = _engine()
    try:
        pool = torch.from_numpy(vols["v"]).cuda()
        e.set_head_precision("f32")
        out = e.heads(pool, pool, lidx=[0, 1, 2], ridx=[3, 3, 3], want_logit=True)
        ws = _ws(e, "f32")
        o2, o3 = (t.cpu().numpy() for t in e.debug_head_activations(3))
        _check_first3(out, vols)
    finally:
        e.close()
    for p in range(3):
        for got, want in ((o2[p], vols["o2"][p]), (o3[p], vols["o3"][p])):
            assert np.max(np.abs(got - np.reshape(want, got.shape))) <= 2e-5 * np.max(np.abs(want)), p
    _pin("f32", ws)


def test_width_split_head():
    """The f16x3 kernels of the fp32 route (set_head_width_split) at W = 45 on 3 pairs: the layout with the per-pair scales; every stage
    within the f16x3 bound of tests/test_gpu_split_width.py."""
    fw = 45
    h, wi = R.GEOMS[(fw, 15)]
    cfg = dict(CFG, inputShape=[h, wi], leg_output_width=fw, additional_unsymmetric_layer3a=False)
    w = S.make_test_weights(4, seed=0, model_cfg=cfg, feat_w=fw)
    rng = np.random.default_rng(45)
    v = np.maximum(rng.normal(0.3, 1.0, size=(3, fw, 128)), 0).astype(np.float32)
    li, ri = [0, 1, 2], [1, 2, 0]
    e = _engine(h, wi, 4, w, cfg)
    try:
        assert e.feat_w == fw
        ft = torch.from_numpy(v).cuda()
        e.set_head_width_split(True)
        out = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True)
        ws = _ws(e, "width_split45")
        o2, o3 = (t.cpu().numpy() for t in e.debug_head_activations(3))
        lg, ov = out["logit"].cpu().numpy(), out["overlap"].cpu().numpy()
    finally:
        e.close()
    for p, (i, j) in enumerate(zip(li, ri)):
        hd = SR.head_pair_split(v[i], v[j], w)
        B = SR.bounds(hd, w)
        rat = {"o2": E.ratio(o2[p], hd["o2"], B["o2"]), "o3": E.ratio(o3[p], hd["o3"], B["o3"]),
               "logit": E.ratio(lg[p], hd["logit"], B["logit"]), "overlap": E.ratio(ov[p], hd["overlap"], B["overlap"])}
        assert all(x <= 1.0 for x in rat.values()), (p, rat)
    _pin("width_split45", ws)


def test_generic_conv1size():
    """conv1size 10 at W = 45 on 2 pairs: the general fp32 route (out1 | o2 | o3)."""
    from tests import test_gpu_feature_width as FW
    fw, s = 45, 10
    h, wi = R.GEOMS[(fw, s)]
    w = R.make_weights(fw, s)
    rng = np.random.default_rng(10)
    v = np.maximum(rng.normal(0.3, 1.0, size=(3, fw, 128)), 0).astype(np.float32)
    li, ri = [0, 2], [1, 0]
    e = _engine(h, wi, 4, w, R.model_cfg(fw, s))
    try:
        assert e.feat_w == fw and e.conv1size == s
        ft = torch.from_numpy(v).cuda()
        out = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True, want_corr=True)
        ws = _ws(e, "generic_s10")
    finally:
        e.close()
    FW._check_heads(out, v[li], v[ri], w, conv1size=s)
    _pin("generic_s10", ws)


@pytest.mark.parametrize("compact,case", [(True, "segments_compact"), (False, "segments_plain")])
def test_heads_segments(compact, case):
    """3 segments, 7 pairs: compaction on -> one segmented pass (per-segment query state behind the sub-chunk block); off -> one
    indexed pass.  == each segment alone in its 1-vs-N form, bit for bit."""
    from tests import test_gpu_batch_queries as BQ
    e = _engine(weights=S.make_trained_like_weights(4))
    try:
        pool = torch.from_numpy(BQ._pool(k=8)).cuda()
        spec, dc = e.spectrum(pool), e.delta_cache(pool)
        offs, q, cand = np.array([0, 2, 3, 7], np.int64), np.array([1, 0, 5], np.int32), np.array([0, 0, 4, 7, 5, 5, 2], np.int32)
        e.set_head_compaction(compact)
        got = e.heads_segments(pool, pool, cand, q, offs, spec_pool=spec, spec_q=spec, dcache_pool=dc, want_logit=True, want_corr=True)
        ws = _ws(e, case)
        BQ._equal(got, BQ._per_query(e, pool, pool, offs, q, cand, spec, spec, dc), case)
    finally:
        e.close()
    _pin(case, ws)


# ---- training -------------------------------------------------------------------------------------------------------------------
def test_delta_head_grad():
    """One pair block and one pair: two blocks of partials.  == the call cut into chunks of one block, bit for bit; overlap within
    its fp64 bound."""
    case = (45, 15, R.PAIR_BLOCK + 1, "idx", "sigmoid")
    assert case in R.CASES
    c, ref = R.reference(case)
    h, wi = R.GEOMS[(45, 15)]
    e = _engine(h, wi, 4, c["weights"], R.model_cfg(45, 15))
    try:
        pool, right = torch.from_numpy(c["pool"]).cuda(), torch.from_numpy(c["right"]).cuda()
        kw = dict(lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"])
        out = e.delta_head_grad(pool, right, c["targets"], **kw)
        ws = _ws(e, "delta_head_grad")
        e.set_head_pipeline(chunk_pairs=R.PAIR_BLOCK)
        chunked = e.delta_head_grad(pool, right, c["targets"], **kw)
        for k in ("flat", "loss", "overlap"):
            assert torch.equal(out[k], chunked[k]), k
        y = out["overlap"].cpu().numpy()
    finally:
        e.close()
    assert np.all(np.abs(y.astype(np.float64) - ref["y"]) <= R.overlap_bounds(c, ref))
    _pin("delta_head_grad", ws)


def test_heads_feature_grad_with_yaw_loss():
    """2 pairs at W = 360, both losses, no head_grad output (the running sums live in the scratch): the Delta gradient's layout, then
    the yaw gradient's in the same block.  Overlap and correlation logits within their fp64 bounds; the same bits twice."""
    case = (360, 15, 2, "idx", "sigmoid")
    assert case in F.CASES
    c, ref = F.reference(case, grad=False)
    h, wi = R.GEOMS[(360, 15)]
    e = _engine(h, wi, 4, c["weights"], R.model_cfg(360, 15))
    try:
        pool, right = torch.from_numpy(c["pool"]).cuda(), torch.from_numpy(c["right"]).cuda()
        args = (pool, right, c["targets"], c["bins"])
        kw = dict(lidx=c["lidx"], ridx=c["ridx"], loss=c["loss"])
        out = e.heads_feature_grad(*args, **kw)
        ws = _ws(e, "heads_feature_grad")
        again = e.heads_feature_grad(*args, **kw)
        for k in ("dfeat_l", "dfeat_r", "loss", "overlap", "corr"):
            assert torch.equal(out[k], again[k]), k
        y, z = out["overlap"].cpu().numpy(), out["corr"].cpu().numpy()
        assert float(out["loss_yaw"]) != 0.0 and bool(torch.any(out["dfeat_l"])) and bool(torch.any(out["dfeat_r"]))
    finally:
        e.close()
    assert np.all(np.abs(y.astype(np.float64) - ref["y"]) <= R.overlap_bounds(c, ref))
    la, ra = torch.tensor(np.abs(c["l"]), dtype=torch.float64), torch.tensor(np.abs(c["r"]), dtype=torch.float64)
    assert np.all(np.abs(z.astype(np.float64) - ref["z"]) <= 2.0 * E.U32 * F.corr_logits(la, ra).numpy())
    _pin("heads_feature_grad", ws)


# ---- the leg --------------------------------------------------------------------------------------------------------------------
def test_leg_one_scan(fixture_npz, nn_golden):
    e = _engine()
    try:
        img = S.stack(fixture_npz["range_0"], fixture_npz["normal_0"], fixture_npz["intensity_0"], S.flags_of(4))[None]
        fv = e.leg(torch.from_numpy(np.ascontiguousarray(img)).cuda())
        ws = _ws(e, "leg")
        fv = fv.cpu().numpy()
    finally:
        e.close()
    want = nn_golden["fv_c4"][0].reshape(fv.shape)
    assert np.max(np.abs(fv - want)) <= 2e-5 * np.max(np.abs(want))
    _pin("leg", ws)


def _within_4T(name, gpu, g32, g64):
    g64 = np.asarray(g64, np.float64)
    T = float(np.max(np.abs(np.asarray(g32, np.float64) - g64)))
    err = float(np.max(np.abs(np.asarray(gpu, np.float64).reshape(g64.shape) - g64)))
    assert np.all(np.isfinite(np.asarray(gpu))) and err <= 4 * T, (name, err, T)


def test_leg_backward_one_scan():
    """leg_forward_train + leg_backward on one scan of the W = 45 leg: every gradient within 4 T of fp64 (tests/test_gpu_leg_train.py)."""
    W = 45
    cfg = R.model_cfg(W, 15)
    h, wi = R.GEOMS[(W, 15)]
    rng = np.random.default_rng([W, 1, 5])
    weights = L.leg_weights(4, cfg, seed=W, feat_w=W)
    images = L.make_images(rng, 1, h, wi, 4)
    e = _engine(h, wi, 4, weights, cfg)
    try:
        x = torch.from_numpy(images).cuda()
        acts = e.leg_forward_train(x)
        assert e.workspace_bytes() == 0
        host = [a.cpu().numpy() for a in acts]
        dfeat = L.random_dfeat(rng, host[-1].reshape(1, W, 128))
        g = e.leg_backward(x, acts, torch.from_numpy(dfeat).cuda())
        ws = _ws(e, "leg_backward")
        got = {name: g[name].cpu().numpy() for name in L.leg_names(4, cfg)}
    finally:
        e.close()
    masks = [a > 0 for a in host]
    g64, _ = L.leg_grads(weights, images, dfeat, cfg, torch.float64, masks)
    g32, _ = L.leg_grads(weights, images, dfeat, cfg, torch.float32, masks)
    for name in L.leg_names(4, cfg):
        _within_4T(name, got[name], g32[name], g64[name])
    _pin("leg_backward", ws)


def test_debug_conv_grad_one_layer():
    cfg = R.model_cfg(45, 15)
    weights = L.leg_weights(4, cfg, seed=0, feat_w=45)
    li = 2
    l = WT.leg_layers(4, cfg)[li]
    x, dout = G.backward_data(li, l, "odd")
    e = _engine(32, 247, 4, weights, cfg)
    try:
        xt, dt = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
        e.set_leg_precision("f32")
        out = e.debug_conv(li, xt)
        assert e.workspace_bytes() == 0
        g = e.debug_conv_grad(li, xt, out, dt)
        ws = _ws(e, "debug_conv_grad")
        mask = (out > 0).cpu().numpy()
        got = {k: g[k].cpu().numpy() for k in ("din", "dkernel", "dbias")}
    finally:
        e.close()
    kern, bias = weights[l.name + "/kernel"], weights[l.name + "/bias"]
    r64 = L.layer_grads(kern, bias, x, mask, dout, (l.sh, l.sw), torch.float64)
    r32 = L.layer_grads(kern, bias, x, mask, dout, (l.sh, l.sw), torch.float32)
    for k in ("din", "dkernel", "dbias"):
        _within_4T(k, got[k], r32[k], r64[k])
    _pin("debug_conv_grad", ws)


# ---- projection -----------------------------------------------------------------------------------------------------------------
def test_project_with_index_image(fixture_npz):
    """2 small clouds with the index image: keys | kept-point numbering | block counts.  Every image equals the CPU oracle's."""
    from overlapnet_amd import preprocess as P
    clouds = [fixture_npz["points_0"][:1000], fixture_npz["points_1"][:700]]
    e = _engine()
    try:
        r = P.project_scans(clouds, engine=e, want=("range", "idx"))
        ws = _ws(e, "project_idx")
        rng, idx = r["range"].cpu().numpy(), r["idx"].cpu().numpy()
    finally:
        e.close()
    for i, pts in enumerate(clouds):
        o_rng, _, _, o_idx = O.range_projection(pts)
        assert np.array_equal(rng[i], o_rng) and np.array_equal(idx[i], o_idx), i
    _pin("project_idx", ws)
