"""GPU (MI355X): the split (f16x3) Delta head at feature widths other than 360 (csrc/delta_head_w_f16x3.hip, opt-in through
`OvnEngine.set_head_width_split` / `config['width_precision'] = 'split'`), element by element against the fp64 head with the derived
f16x3 bound of oracle/error_bounds.py (tests/_split_width_ref.py adds the c_conv1 entry the oracle leaves out off 360).

How the split kernels tile, with G = W // 15 and R = 15 G (the rule of ovn_delta_w_split_c12_forward):
    delta_c12_w_split_kernel<MT>   MT = ceil(G / 16) GEMM2 row tiles;  ceil(ceil(R / 16) / 24) passes over the row tiles of GEMM1
WIDTHS: 45 (G = 3), 59 (14 unread tail columns), 371 (32 x 900 scans), 385, 422 (64 x 1024 scans), 512 (G = 34), and one width on
each side of every switch: MT 1 | 2 at 254 | 255, MT 2 | 3 at 494 | 495, one pass | two at 384 | 390 (R = 375 | 390; 24 row tiles
hold R <= 384).  Inputs are the sets of tests/test_gpu_width_edges.py.  Each test prints its worst err / bound per stage."""
import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd import weights as WT
from tests import _split_width_ref as SR
from tests import test_gpu_width_edges as WE
from tools import synthetic as S


def gpu(f):
    return pytest.mark.gpu(pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")(f))


# W -> (input (H, W), additional_unsymmetric_layer3a) of a leg that produces it
GEOM = {fw: (WE.WIDTHS[fw], False) for fw in (45, 59, 254, 255, 384, 385, 390, 494, 495, 512)}
GEOM[371] = ((32, 900), False)
GEOM[422] = ((64, 1024), True)
WIDTHS = sorted(GEOM)
# W -> (G, MT, passes)
TILING = {45: (3, 1, 1), 59: (3, 1, 1), 254: (16, 1, 1), 255: (17, 2, 1), 371: (24, 2, 1), 384: (25, 2, 1), 385: (25, 2, 1),
          390: (26, 2, 2), 422: (28, 2, 2), 494: (32, 2, 2), 495: (33, 3, 2), 512: (34, 3, 2)}
STAGES = ("o2", "o3", "logit", "overlap")


def _tiling(fw):
    """(G, MT, passes) as ovn_delta_w_split_c12_forward and its kernel choose them."""
    g = fw // 15
    return g, -(-g // 16), -(-(-(-15 * g // 16)) // 24)


def test_widths_reach_every_tiling():
    for fw in WIDTHS:
        assert _tiling(fw) == TILING[fw], fw
        (h, w), a3 = GEOM[fw]
        assert WT.leg_output_shape(h, w, WT.leg_layers(4, _cfg(fw))) == (1, fw, 128)
    assert {t[1:] for t in TILING.values()} == {(1, 1), (2, 1), (2, 2), (3, 2)}
    for a, b in ((254, 255), (494, 495), (384, 390)):           # both sides of every switch
        assert TILING[a][1:] != TILING[b][1:]


def _cfg(fw):
    (h, w), a3 = GEOM[fw]
    return dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=fw, additional_unsymmetric_layer3a=a3)


_W = {}


def _weights(fw):
    if fw not in _W:
        _W[fw] = S.make_test_weights(4, seed=0, model_cfg=_cfg(fw), feat_w=fw)
    return _W[fw]


@pytest.fixture(scope="module")
def engines():
    from overlapnet_amd.engine import OvnEngine
    made = {}

    def get(fw):
        if fw not in made:
            (h, w), _ = GEOM[fw]
            e = OvnEngine(h, w, 4)
            try:
                e.load_weights(_weights(fw), _cfg(fw))
                assert e.feat_w == fw
            except Exception:
                e.close()
                raise
            made[fw] = e
        return made[fw]
    yield get
    for e in made.values():
        e.close()


def _run(e, ft, li, ri, prec, split):
    e.set_head_precision(prec)
    e.set_head_width_split(split)
    try:
        out = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True, want_corr=True)
        out["o2"], out["o3"] = e.debug_head_activations(len(li))
    finally:
        e.set_head_precision("f16x3")
        e.set_head_width_split(False)
    return out


# ---- 1-3: every stage of every pair against the bound; the yaw head and the other modes keep their bits ---------------------------
@gpu
@pytest.mark.parametrize("fw", WIDTHS, ids=lambda fw: "W%d" % fw)
def test_stages_against_the_f16x3_bound(engines, fw):
    e = engines(fw)
    w = _weights(fw)
    g = fw // 15
    worst = {}
    differs = False
    for name, v in WE._sets(fw).items():
        pairs = WE._pairs(name, v.shape[0], fw)
        ft = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        li, ri = [p[0] for p in pairs], [p[1] for p in pairs]
        exact = _run(e, ft, li, ri, "f32", False)                      # today's fp32 results
        got = _run(e, ft, li, ri, "f16x3", True)
        for k in ("yaw", "corr"):                                      # 2: the yaw head does not change by a bit
            assert torch.equal(got[k], exact[k]), (name, k)
        for prec, split in (("f16x3", False), ("f32", True), ("bf16x3", True), ("bf16x3", False)):   # 3: everything else is fp32
            other = _run(e, ft, li, ri, prec, split)
            for k in ("overlap", "logit", "o2", "o3", "yaw", "corr"):
                assert torch.equal(other[k], exact[k]), (name, prec, split, k)
        differs = differs or not torch.equal(got["o2"], exact["o2"])
        o2, o3 = got["o2"].cpu().numpy(), got["o3"].cpu().numpy()
        lg, ov = got["logit"].cpu().numpy(), got["overlap"].cpu().numpy()
        assert o2.shape == (len(pairs), g, g, 128) and o3.shape == (len(pairs), g - 2, g - 2, 256)
        for p, (i, j) in enumerate(pairs):                             # 1: every element of every pair, no tolerance but B
            h = SR.head_pair_split(v[i], v[j], w)
            B = SR.bounds(h, w)
            rat = {"o2": E.ratio(o2[p], h["o2"], B["o2"]), "o3": E.ratio(o3[p], h["o3"], B["o3"]),
                   "logit": E.ratio(lg[p], h["logit"], B["logit"]), "overlap": E.ratio(ov[p], h["overlap"], B["overlap"])}
            for k, x in rat.items():
                worst[k] = max(worst.get(k, 0.0), x)
            bad = {k: x for k, x in rat.items() if not x <= 1.0}
            assert not bad, "[W=%d %s pair %d] over the f16x3 bound: %s" % (fw, name, p, bad)
    print("\n[W=%d G=%d MT=%d passes=%d] f16x3 split route, worst err / bound: %s" % ((fw,) + _tiling(fw) + (WE._fmt(worst),)))
    assert differs, "the switch changed nothing: the split kernels did not run"


@gpu
def test_switch_changes_nothing_at_360():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4)
    try:
        e.load_weights(S.make_test_weights(4, seed=0), S.REFERENCE_MODEL_CFG)
        assert e.feat_w == 360 and e.head_width_split is False
        v = torch.from_numpy(WE._relu(360, 6, 360)).cuda()
        res = {}
        for split in (False, True):
            e.set_head_width_split(split)
            assert e.head_width_split is split
            res[split] = e.heads(v, v[2:3].contiguous(), want_logit=True, want_corr=True)
            res[split]["o2"] = e.debug_head_activations(6)[0]
        for k in ("overlap", "logit", "yaw", "corr", "o2"):
            assert torch.equal(res[True][k], res[False][k]), k
    finally:
        e.close()


# ---- 4: a pair's bits do not depend on the call around it ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fw", WIDTHS, ids=lambda fw: "W%d" % fw)
def test_pair_is_independent_of_its_call(engines, fw):
    """A pair alone, inside a 1024-pair sweep, across chunk borders and through shuffled lidx / ridx
    and as a segment of a batch of queries: the same bits.  The volumes
    differ in range by powers of two and some carry negative values, so the per-pair scales differ along the sweep."""
    e = engines(fw)
    n = 1024
    gen = torch.Generator(device="cuda").manual_seed(fw)
    v = torch.relu(torch.randn((n, fw, 128), device="cuda", generator=gen) + 0.2)
    v = v * torch.pow(2.0, (torch.arange(n, device="cuda") % 7 - 3).float())[:, None, None]
    v[5::13] -= 0.37                                                   # pairs with a shift
    q = v[17:18].contiguous()
    keys = ("overlap", "logit")
    e.set_head_width_split(True)
    try:
        sweep = e.heads(v, q, want_logit=True)
        probe = [0, 5, 17, 18, 511, 512, 1018, 1023]
        for i in probe:
            one = e.heads(v[i:i + 1].contiguous(), q, want_logit=True)
            for k in keys:
                assert torch.equal(one[k], sweep[k][i:i + 1]), (k, i)
        for chunk in (1, 7, 100):
            e.set_head_pipeline(chunk)
            m = 64 if chunk == 1 else n
            d = e.heads(v[:m].contiguous(), q, want_logit=True)
            for k in keys:
                assert torch.equal(d[k], sweep[k][:m]), (k, chunk)
        e.set_head_pipeline(1024)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(fw)).tolist()
        ix = e.heads(v, v, lidx=perm, ridx=[17] * n, want_logit=True)
        pt = torch.tensor(perm, device="cuda")
        for k in keys:
            assert torch.equal(ix[k], sweep[k][pt]), k
        # any right volume through ridx: pair (perm[p], rr[p]) against the same pair alone
        rr = [(3 * p + 1) % n for p in range(16)]
        ix2 = e.heads(v, v, lidx=perm[:16], ridx=rr, want_logit=True)
        for p in (0, 7, 15):
            one = e.heads(v[perm[p]:perm[p] + 1].contiguous(), v[rr[p]:rr[p] + 1].contiguous(), want_logit=True)
            for k in keys:
                assert torch.equal(one[k], ix2[k][p:p + 1]), (k, p)
        # a batch of queries (ovn_heads_segments), with passes that cut segments, against the per-query sweeps
        offs, qi, cand = WE._segments(np.random.default_rng(fw), 12, 12)
        pool = v[:12].contiguous()
        want = [e.heads(pool, pool[int(qi[b]):int(qi[b]) + 1], lidx=cand[int(offs[b]):int(offs[b + 1])], want_logit=True)
                for b in range(len(qi)) if offs[b] < offs[b + 1]]
        for chunk in (1024, 7):
            e.set_head_pipeline(chunk)
            got = e.heads_segments(pool, pool, cand, qi, offs, want_logit=True)
            for k in keys:
                assert torch.equal(got[k], torch.cat([x[k] for x in want])), (k, chunk)
    finally:
        e.set_head_pipeline(1024)
        e.set_head_width_split(False)


# ---- 5: Infer -------------------------------------------------------------------------------------------------------------------------
def _write_cues(root, fw, n):
    """n synthetic range / normal images of the leg's input size under root/07 (a smooth scene, shifted and perturbed per frame)."""
    import os
    (h, w), _ = GEOM[fw]
    seq = os.path.join(root, "07")
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(seq, sub), exist_ok=True)
    rng = np.random.default_rng(fw)
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 2 * np.pi, w, endpoint=False), indexing="ij")
    for i in range(n):
        d = (12 + 8 * np.sin(3 * xx + 0.4 * i) * np.cos(2 * yy) + 3 * np.cos(7 * xx - 0.3 * i) + rng.normal(0, 0.2, (h, w)))
        nm = np.stack([np.cos(xx + 0.2 * i), np.sin(xx + 0.2 * i), 0.3 * np.cos(5 * yy + i)], axis=-1) + rng.normal(0, 0.05, (h, w, 3))
        nm /= np.linalg.norm(nm, axis=-1, keepdims=True)
        np.save(os.path.join(seq, "depth", "%06d.npy" % i), d.astype(np.float32))
        np.save(os.path.join(seq, "normal", "%06d.npy" % i), nm.astype(np.float32))


def _infer_cfg(fw, root, **extra):
    cfg = {"model": _cfg(fw), "infer_seqs": "07", "data_root_folder": str(root), "use_depth": True, "use_normals": True,
           "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16,
           "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


@gpu
@pytest.mark.parametrize("fw", [422, 371], ids=lambda fw: "W%d" % fw)
def test_infer_with_width_precision_split(fw, tmp_path):
    """inputShape 64 x 1024 (W = 422) and 32 x 900 (W = 371): infer_multiple is the engine-level sweep on the same volumes bit for
    bit, infer_top_k and infer_multiple_batch agree with it, and the overlaps sit within B_f16x3 + B_f32 of the 'exact' run of the
    same config."""
    from overlapnet_amd.infer import Infer
    w = _weights(fw)
    n = 6
    _write_cues(str(tmp_path / "data"), fw, n)
    refs = list(range(n - 1))
    res = {}
    for mode in ("split", "exact"):
        inf = Infer(_infer_cfg(fw, tmp_path / "data", width_precision=mode), weights=w)
        try:
            assert inf.feat_w == fw and inf.engine.head_width_split is (mode == "split")
            for i in range(n):                                        # frames in order: the cache index is the frame id
                r = inf.infer_multiple(i, list(range(i)))
            ov, yaw = np.asarray(r[0], np.float32).reshape(-1), np.asarray(r[1]).reshape(-1)
            vols = np.array(inf.feature_volumes)[:, 0]
            assert vols.shape == (n, fw, 128)
            ft = torch.from_numpy(vols).cuda()
            sweep = inf.engine.heads(ft[:n - 1].contiguous(), ft[n - 1:].contiguous())
            assert np.array_equal(ov, sweep["overlap"].cpu().numpy()) and np.array_equal(yaw, sweep["yaw"].cpu().numpy())
            inf.feature_volumes = [vols[i][None] for i in range(n - 1)]
            top = inf.infer_top_k(n - 1, refs, k=3, overlap_thres=None)
            order = sorted(refs, key=lambda i: (-float(ov[i]), i))[:3]
            assert [t[0] for t in top] == order
            for rid, o, y in top:
                assert np.float32(o) == ov[rid] and int(y) == int(yaw[rid])
            batch = inf.infer_multiple_batch([n - 1, 2], [refs, [0, 1]])
            assert np.array_equal(np.asarray(batch[0][0], np.float32).reshape(-1), ov)
            assert np.array_equal(np.asarray(batch[0][1]).reshape(-1), yaw)
            two = inf.engine.heads(ft[:2].contiguous(), ft[2:3].contiguous())
            assert np.array_equal(np.asarray(batch[1][0], np.float32).reshape(-1), two["overlap"].cpu().numpy())
            res[mode] = (ov.astype(np.float64), vols)
        finally:
            inf.close()
    assert np.array_equal(res["split"][1], res["exact"][1])             # the leg does not follow the key
    assert not np.array_equal(res["split"][0], res["exact"][0]), "width_precision changed nothing"
    vols = res["split"][1]
    worst = 0.0
    for i in refs:
        h = SR.head_pair_split(vols[i], vols[n - 1], w)
        b = SR.bounds(h, w)["overlap"] + E.head_bounds(h, w, "f32")["overlap"]
        worst = max(worst, abs(res["split"][0][i] - res["exact"][0][i]) / b)
    print("\n[W=%d Infer] |overlap split - overlap exact| / (B_f16x3 + B_f32): worst %.3g" % (fw, worst))
    assert worst <= 1.0
