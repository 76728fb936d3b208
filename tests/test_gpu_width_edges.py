"""GPU (MI355X): the fp32 heads (delta_head.hip, corr_head.hip) at the ends of every tile-shape range they choose from the feature
width W, and at the shipped 360 columns, against the elementwise fp64 bounds of oracle/error_bounds.py (the standard the
split-operand paths at W = 360 are held to in tests/test_gpu_error_bounds.py).

How the kernels tile, with G = W // 15 and R = 15 G (the rule of ovn_delta_forward / ovn_corr_forward):
    delta_c12_kernel<T, MT>   T = 3 row tiles per wave for R <= 384, else 4;  MT = ceil(G / 16) GEMM2 row tiles
    corr_head_kernel<T, NORM> T = 3 for W <= 384, else 4;  NORM with a normalisation mode
WIDTHS holds one end of every range: <3,1> 45 / 254, <3,2> 255 / 375 / 384 (R = 375 at both), <4,2> 390 / 494, <4,3> 495 / 512;
360 itself (<3,2>, correlation <3,*>: there the fp32 kernels are head precision "f32", the other two precisions have kernels and
tests of their own); the correlation's <3,*> / <4,*> edge at 384 / 385; G = 3 at 45 (c_conv3 to 1 x 1, a 256-input Dense); 14 unread tail columns at
59; a one-column last Gram panel at 385 and a 13-column one at 45; 22 normalisation blocks (the most) at 512.  Each engine is built
from a real leg geometry (32 x N scans; 64 x N with additional_unsymmetric_layer3a for the A3 cases).  Each test prints its worst
err / bound per stage (<= 1 passes)."""
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from oracle import overlapnet_oracle as O
from overlapnet_amd import weights as WT
from tests import _corr_norm_ref as R
from tools import synthetic as S


def gpu(f):
    return pytest.mark.gpu(pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")(f))


# W -> input (H, W) of a leg that produces it, additional_unsymmetric_layer3a off (but on at 360: 64 x 900 is the shipped geometry)
WIDTHS = {45: (32, 247), 59: (32, 275), 254: (32, 665), 255: (32, 667), 360: (64, 900), 375: (32, 907), 384: (32, 925),
          385: (32, 927), 390: (32, 937), 494: (32, 1145), 495: (32, 1147), 512: (32, 1181)}
A3_GEOM = {45: (64, 269), 360: (64, 900), 512: (64, 1203)}   # widths with additional_unsymmetric_layer3a on
# W -> (G, Delta T, Delta MT, correlation T), the table of the issue this file was written for
TILING = {45: (3, 3, 1, 3), 59: (3, 3, 1, 3), 254: (16, 3, 1, 3), 255: (17, 3, 2, 3), 360: (24, 3, 2, 3), 375: (25, 3, 2, 3),
          384: (25, 3, 2, 3), 385: (25, 3, 2, 4), 390: (26, 4, 2, 4), 494: (32, 4, 2, 4), 495: (33, 4, 3, 4), 512: (34, 4, 3, 4)}
NORM_WIDTHS = (45, 360, 385, 512)
PRECISIONS = ("f32", "f16x3", "bf16x3")


def _tiling(fw):
    """(G, T, MT, correlation T) as ovn_delta_forward and ovn_corr_forward choose them."""
    g = fw // 15
    return g, 3 if 15 * g <= 384 else 4, -(-g // 16), 3 if fw <= 384 else 4


def test_widths_reach_every_instantiation():
    """The widths above are the ends of the ranges of the table, and together they reach all eight instantiations."""
    for fw in WIDTHS:
        assert _tiling(fw) == TILING[fw], fw
        h, w = WIDTHS[fw]
        assert WT.leg_output_shape(h, w, WT.leg_layers(4, _cfg(fw))) == (1, fw, 128)
    for fw, (h, w) in A3_GEOM.items():
        assert WT.leg_output_shape(h, w, WT.leg_layers(4, _cfg(fw, a3=True))) == (1, fw, 128)
    assert {(t, mt) for _, t, mt, _ in TILING.values()} == {(3, 1), (3, 2), (4, 2), (4, 3)}
    corr = {(TILING[fw][3], False) for fw in WIDTHS} | {(TILING[fw][3], True) for fw in NORM_WIDTHS}
    assert corr == {(3, False), (3, True), (4, False), (4, True)}
    for t, mt in ((3, 1), (3, 2), (4, 2), (4, 3)):           # both ends of every Delta range
        ws = [fw for fw in WIDTHS if TILING[fw][1:3] == (t, mt)]
        assert len(ws) >= 2, (t, mt)
    # the shipped 360 columns: delta_c12_kernel<3, 2>, corr_head_kernel<3, false> and, with a mode, <3, true>
    assert TILING[360] == (24, 3, 2, 3) and 360 in NORM_WIDTHS and 360 % 24 == 0
    assert 59 - 15 * (59 // 15) == 14 and 385 % 16 == 1 and 45 % 16 == 13 and -(-512 // 24) == 22


def _cfg(fw, a3=False, **extra):
    a3 = a3 or fw == 360
    h, w = A3_GEOM[fw] if a3 else WIDTHS[fw]
    return dict(S.REFERENCE_MODEL_CFG, inputShape=[h, w], leg_output_width=fw, additional_unsymmetric_layer3a=a3, **extra)


_W = {}


def _weights(fw, seed=0):
    if (fw, seed) not in _W:
        _W[(fw, seed)] = S.make_test_weights(4, seed=seed, model_cfg=_cfg(fw), feat_w=fw)
    return _W[(fw, seed)]


def _engine(fw, w=None, a3=False, **extra):
    from overlapnet_amd.engine import OvnEngine
    h, wi = A3_GEOM[fw] if a3 else WIDTHS[fw]                     # (the same entry at 360)
    e = OvnEngine(h, wi, 4)
    try:
        e.load_weights(_weights(fw) if w is None else w, _cfg(fw, a3, **extra))
        assert e.feat_w == fw
    except Exception:
        e.close()
        raise
    return e


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(fw):
        if fw not in made:
            made[fw] = _engine(fw)
        return made[fw]
    yield get
    for e in made.values():
        e.close()


def _relu(fw, k, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, fw, 128)), 0).astype(np.float32)
    for i in range(k):
        v[i][:, rng.permutation(128)[:32]] = 0                   # dead channels
    return v * np.float32(scale)


def _sets(fw):
    sets = {"relu": _relu(fw, 4, fw), "x300": _relu(fw, 3, fw + 1, 300.0)}
    sets.update(E.value_edge_sets(seed=fw, width=fw))
    return sets


def _pairs(name, k, fw):
    pairs = [(i, 0) for i in range(k)] + [(0, 1)]
    if name == "subnormal":
        pairs.append((1, 1))                                       # two volumes of subnormals
    return pairs[:3] + pairs[-1:] if fw > 384 and len(pairs) > 4 else pairs


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fmt(worst):
    return {k: "%.3g" % v for k, v in sorted(worst.items())}


def _check_pairs(tag, out, o2, o3, v, pairs, w, worst, corr_bound=None):
    lg, ov = out["logit"].cpu().numpy(), out["overlap"].cpu().numpy()
    g_corr, g_yaw = out["corr"].cpu().numpy(), out["yaw"].cpu().numpy()
    for p, (i, j) in enumerate(pairs):
        h = E.head_pair(v[i], v[j], w)
        B = E.head_bounds(h, w, "f32")
        c = E.corr_pair(v[i], v[j]) if corr_bound is None else corr_bound(v[i], v[j])
        rat = {"o2": E.ratio(o2[p], h["o2"], B["o2"]), "o3": E.ratio(o3[p], h["o3"], B["o3"]),
               "logit": E.ratio(lg[p], h["logit"], B["logit"]), "overlap": E.ratio(ov[p], h["overlap"], B["overlap"]),
               "corr": E.ratio(g_corr[p], c["corr"], c["direct"])}
        for k, x in rat.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert R.yaw_ok(g_corr[p], 180 - g_yaw[p], c["corr"], c["direct"]), (tag, p, g_yaw[p])
        assert int(g_yaw[p]) == 180 - int(np.argmax(g_corr[p])), (tag, p)
    bad = {k: x for k, x in worst.items() if not x <= 1.0}
    assert not bad, "[%s] over the bound: %s" % (tag, bad)


# ---- stages against the bound, and the three head precisions -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fw", sorted(WIDTHS), ids=lambda fw: "W%d" % fw)
def test_stages_against_the_bound(engines, fw):
    """o2 and o3 (through ovn_debug_head_activations), the logit, the overlap and every correlation element of every pair against
    the fp32 bound, on ReLU volumes with dead channels, a x300 set and the value-edge sets; off 360 f16x3 and bf16x3 give the f32
    bits (at 360 they are kernels of their own, held to their own bounds in tests/test_gpu_error_bounds.py)."""
    e = engines(fw)
    w = _weights(fw)
    g = fw // 15
    worst = {}
    for name, v in _sets(fw).items():
        pairs = _pairs(name, v.shape[0], fw)
        ft = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        li, ri = [p[0] for p in pairs], [p[1] for p in pairs]
        res = {}
        for prec in PRECISIONS if fw != 360 else PRECISIONS[:1]:
            e.set_head_precision(prec)
            res[prec] = e.heads(ft, ft, lidx=li, ridx=ri, want_logit=True, want_corr=True)
            a2, a3 = e.debug_head_activations(len(pairs))
            res[prec]["o2"], res[prec]["o3"] = a2, a3
        e.set_head_precision("f16x3")
        for prec in PRECISIONS[1:] if fw != 360 else ():            # every precision runs the exact fp32 kernels off 360
            for k in ("overlap", "logit", "yaw", "corr", "o2", "o3"):
                assert torch.equal(res[prec][k], res["f32"][k]), (name, prec, k)
        o2, o3 = res["f32"]["o2"].cpu().numpy(), res["f32"]["o3"].cpu().numpy()
        assert o2.shape == (len(pairs), g, g, 128) and o3.shape == (len(pairs), g - 2, g - 2, 256)
        _check_pairs("W=%d %s" % (fw, name), res["f32"], o2, o3, v, pairs, w, worst)
    print("\n[W=%d G=%d T=%d MT=%d corr T=%d] worst err / bound: %s" % ((fw,) + _tiling(fw) + (_fmt(worst),)))


@gpu
def test_debug_hook_refuses_a_call_of_several_chunks(engines):
    """The hook returns the activations of a call that ran as one chunk only; after several chunks it refuses (OVN_ERR_STATE)
    instead of returning another chunk's values."""
    from overlapnet_amd._lib import OvnError
    e = engines(45)
    v = torch.from_numpy(_relu(45, 5, 3)).cuda()
    try:
        e.set_head_pipeline(2)
        e.heads(v, v[:1])
        with pytest.raises(OvnError, match="call right after ovn_heads"):
            e.debug_head_activations(1)
        e.set_head_pipeline(1024)
        e.heads(v, v[:1])
        o2, o3 = e.debug_head_activations(5)
        with pytest.raises(OvnError, match="call right after ovn_heads"):
            e.debug_head_activations(6)
        assert o2.shape == (5, 3, 3, 128) and o3.shape == (5, 1, 1, 256)
    finally:
        e.set_head_pipeline(1024)


# ---- routes and launch shapes: the same bits ---------------------------------------------------------------------------------------
def _segments(rng, npool, nq):
    from tests.test_gpu_batch_queries import _segments as seg
    return seg(rng, npool, nq)


@gpu
@pytest.mark.parametrize("fw", sorted(WIDTHS), ids=lambda fw: "W%d" % fw)
def test_routes_and_launch_shapes_same_bits(engines, fw):
    e = engines(fw)
    keys = ("overlap", "logit", "yaw", "corr")
    v = torch.from_numpy(_relu(fw, 12, 7 * fw)).cuda()
    q = v[5:6].contiguous()
    try:
        if fw == 360:
            e.set_head_precision("f32")                             # off 360 every precision runs these kernels
        a = e.heads(v, q, want_logit=True, want_corr=True)                                      # 1-vs-N
        b = e.heads(v, v, lidx=list(range(12)), ridx=[5] * 12, want_logit=True, want_corr=True)  # the same pairs by index
        parts = [e.heads(v[i:i + 3].contiguous(), q, want_logit=True, want_corr=True) for i in range(0, 12, 3)]   # small sweeps
        c = e.corr_head(v, q, want_corr=True)
        for k in keys:
            assert torch.equal(a[k], b[k]), k
            assert torch.equal(a[k], torch.cat([p[k] for p in parts])), k
        assert torch.equal(c["corr"], a["corr"]) and torch.equal(c["yaw"], a["yaw"])
        for chunk in (1, 7, 1024):
            e.set_head_pipeline(chunk)
            d = e.heads(v, q, want_logit=True, want_corr=True)
            for k in keys:
                assert torch.equal(a[k], d[k]), (k, chunk)
        # batches of queries: heads_segments and top_k_segments against the per-query loop, with passes that cut segments
        rng = np.random.default_rng(fw)
        offs, qi, cand = _segments(rng, 12, 12)
        want = []
        for bq in range(len(qi)):
            o0, o1 = int(offs[bq]), int(offs[bq + 1])
            if o0 < o1:
                want.append(e.heads(v, v[int(qi[bq]):int(qi[bq]) + 1], lidx=cand[o0:o1], want_logit=True, want_corr=True))
        want = {k: torch.cat([x[k] for x in want]) for k in keys}
        for chunk in (1024, 7):
            e.set_head_pipeline(chunk)
            got = e.heads_segments(v, v, cand, qi, offs, want_logit=True, want_corr=True)
            for k in keys:
                assert torch.equal(got[k], want[k]), (k, chunk)
        tk = e.top_k_segments(got["overlap"], offs, got["yaw"], 5, 0.3)
        for bq in range(len(qi)):
            o0, o1 = int(offs[bq]), int(offs[bq + 1])
            one = e.top_k(got["overlap"][o0:o1].contiguous(), got["yaw"][o0:o1].contiguous(), 5, 0.3)
            assert torch.equal(tk[bq], one), bq
    finally:
        e.set_head_pipeline(1024)
        e.set_head_precision("f16x3")


# ---- known answer ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fw", sorted(WIDTHS), ids=lambda fw: "W%d" % fw)
def test_known_answer_yaw_every_normalize_mode(engines, fw):
    """r = roll(l, s): yaw = 180 - known_bin(s, W) for s in {0, 1, W // 2, W - 1}, in every normalisation mode."""
    e = engines(fw)
    x = _relu(fw, 1, 11 * fw)[0]
    shifts = (0, 1, fw // 2, fw - 1)
    rs = torch.from_numpy(np.stack([R.rolled(x, s) for s in shifts])).cuda()
    lt = torch.from_numpy(x[None]).cuda()
    want = [180 - R.known_bin(s, fw) for s in shifts]
    try:
        for mode in R.MODES:
            e.set_corr_normalization(mode)
            out = e.heads(lt, rs, lidx=[0] * 4, ridx=[0, 1, 2, 3], want_corr=True)
            assert out["yaw"].cpu().tolist() == want, (mode, out["yaw"].cpu().tolist(), want)
            assert e.corr_head(lt, rs, lidx=[0] * 4, ridx=[0, 1, 2, 3])["yaw"].cpu().tolist() == want, mode
    finally:
        e.set_corr_normalization("none")


# ---- normalize modes and negateDiffs ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fw", NORM_WIDTHS, ids=lambda fw: "W%d" % fw)
def test_normalize_modes_and_negate_diffs(fw):
    """W = 45 and 360 run corr_head_kernel<3, true>, 385 and 512 <4, true>: every mode against corr_norm_pair's direct bound on
    edge_volume (its 2^100 channel zeroed in mode 'none', where the products leave fp32); DeltaLayer negateDiffs against the bound
    of the negated c_conv1 kernel, with the Delta head's bits the same in every mode."""
    ev = np.stack([R.edge_volume(fw + i, fw) for i in range(3)])
    rv = _relu(fw, 3, 5 * fw)
    pairs = [(0, 1), (1, 2), (2, 0), (1, 1)]
    li, ri = [p[0] for p in pairs], [p[1] for p in pairs]
    w = _weights(fw, seed=3)
    wn = dict(w)
    wn["c_conv1/kernel"] = -w["c_conv1/kernel"]
    for negate in (False, True):
        e = _engine(fw, w, deltaLayer_negateDiffs=negate)
        try:
            e.set_head_precision("f32")
            base = e.heads(_t(rv), _t(rv), lidx=li, ridx=ri, want_logit=True, want_corr=True)
            o2, o3 = [t.cpu().numpy() for t in e.debug_head_activations(len(pairs))]
            wk = {}
            _check_pairs("W=%d negate=%s" % (fw, negate), base, o2, o3, rv, pairs, wn if negate else w, wk)
            print("\n[W=%d negateDiffs=%s] worst err / bound: %s" % (fw, negate, _fmt(wk)))
            for mode in R.MODES:
                e.set_corr_normalization(mode)
                v = ev.copy()
                if mode == "none":
                    v[:, :, 12] = 0
                out = e.heads(_t(v), _t(v), lidx=li, ridx=ri, want_logit=True, want_corr=True)
                c_only = e.corr_head(_t(v), _t(v), lidx=li, ridx=ri, want_corr=True)
                assert torch.equal(c_only["corr"], out["corr"]) and torch.equal(c_only["yaw"], out["yaw"])
                again = e.heads(_t(rv), _t(rv), lidx=li, ridx=ri, want_logit=True)
                assert torch.equal(again["overlap"], base["overlap"]) and torch.equal(again["logit"], base["logit"]), mode
                corr, yaw = out["corr"].cpu().numpy(), out["yaw"].cpu().numpy()
                worst = 0.0
                for p, (i, j) in enumerate(pairs):
                    ref = R.corr_norm_pair(v[i], v[j], mode)
                    rat = E.ratio(corr[p], ref["corr"], ref["direct"])
                    worst = max(worst, rat)
                    assert rat <= 1.0, (fw, mode, negate, p, rat)
                    assert R.yaw_ok(corr[p], 180 - int(yaw[p]), ref["corr"], ref["direct"]), (fw, mode, negate, p)
                print("[W=%d %s negateDiffs=%s] corr worst err / bound: %.3g" % (fw, mode, negate, worst))
        finally:
            e.close()


# ---- the leg -----------------------------------------------------------------------------------------------------------------------
LEGS = [(45, False), (45, True), (512, False), (512, True)]


def leg_against_the_bound(cfg, h, wi, fw, tag, layers=True):
    """The leg of model section `cfg` at input h x wi (feature width fw) on two scans, in both leg precisions: its output against the
    bound of leg_with_bounds, and with `layers` every layer in isolation (ovn_debug_conv on a context holding that layer alone) on
    the fp32 rounding of its exact input.  Prints the worst err / bound per precision and layer."""
    from overlapnet_amd import _lib
    from overlapnet_amd.engine import OvnEngine, _ptr
    rng = np.random.default_rng(h * 10000 + wi)
    imgs = rng.normal(0.5, 1.0, size=(2, h, wi, 4)).astype(np.float32)
    wts = S.make_test_weights(4, seed=0, model_cfg=cfg, feat_w=fw)
    bounds = E.leg_with_bounds(imgs, wts, ("f16x3", "f32"), cfg)
    e = OvnEngine(h, wi, 4)
    try:
        e.load_weights(wts, cfg)
        assert e.feat_w == fw
        for mode in ("f16x3", "f32"):
            e.set_leg_precision(mode)
            out = e.leg(torch.from_numpy(imgs).cuda()).cpu().numpy()
            name, x, B = bounds[mode][-1]
            assert out.shape == (2, fw, 128)
            rt = E.ratio(out, x.reshape(out.shape), B.reshape(out.shape))
            print("\n[leg %dx%d %s %s] worst err / bound of %s: %.3g" % (h, wi, tag, mode, name, rt))
            assert rt <= 1.0, (h, wi, mode, rt)
    finally:
        e.close()
    x = imgs
    hh, ww = h, wi
    for l, (name, ref_out, _) in zip(WT.leg_layers(4, cfg), bounds["f32"]):
        assert l.name == name
        oh, ow = (hh - l.kh) // l.sh + 1, (ww - l.kw) // l.sw + 1
        if layers is True or name in layers:
            el = OvnEngine(hh, ww, l.cin)
            try:
                kt = torch.from_numpy(wts[name + "/kernel"]).cuda()
                bt = torch.from_numpy(wts[name + "/bias"]).cuda()
                st = el._stream()
                _lib.check(el.lib.ovn_add_leg_layer(el._h, name.encode(), _ptr(kt), _ptr(bt), l.kh, l.kw, l.cin, l.cout, l.sh, l.sw, st),
                           "ovn_add_leg_layer")
                xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
                out = torch.empty((x.shape[0], oh, ow, l.cout), dtype=torch.float32, device="cuda")
                ref, B = E.leg_layer_bound(x, wts[name + "/kernel"], wts[name + "/bias"], (l.sh, l.sw))
                for mode in ("f16x3", "f32"):
                    el.set_leg_precision(mode)
                    out.fill_(float("nan"))
                    _lib.check(el.lib.ovn_debug_conv(el._h, 0, _ptr(xt), x.shape[0], hh, ww, _ptr(out), st), "ovn_debug_conv")
                    torch.cuda.synchronize()
                    rt = E.ratio(out.cpu().numpy(), ref, B[mode])
                    print("[leg layer %s %dx%d %s] worst err / bound: %.3g" % (name, hh, ww, mode, rt))
                    assert rt <= 1.0, (name, hh, ww, mode, rt)
            finally:
                el.close()
        x = ref_out.astype(np.float32)
        hh, ww = oh, ow


@gpu
@pytest.mark.parametrize("fw,a3", LEGS, ids=lambda x: str(x))
def test_leg_against_the_bound(fw, a3):
    """The leg at 32 x 247, 64 x 269, 32 x 1181 and 64 x 1203 in both leg precisions: its output against the bound of
    leg_with_bounds, and every layer in isolation (ovn_debug_conv) on the fp32 rounding of its exact input."""
    h, wi = A3_GEOM[fw] if a3 else WIDTHS[fw]
    leg_against_the_bound(_cfg(fw, a3), h, wi, fw, "a3=%s" % a3)


# ---- Infer end to end --------------------------------------------------------------------------------------------------------------
def _write_cues(root, fx, n, h, wi):
    seq = os.path.join(root, "07")
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(seq, sub), exist_ok=True)
    imgs = []
    for i in range(n):
        s, shift = i % 2, 40 * (i // 2)
        d, nm = [np.roll(fx[k % s], shift, axis=1)[::64 // h] for k in ("range_%d", "normal_%d")]
        reps = -(-wi // d.shape[1])                                # tile the columns to the scan width, then crop
        d = np.ascontiguousarray(np.concatenate([d] * reps, axis=1)[:, :wi])
        nm = np.ascontiguousarray(np.concatenate([nm] * reps, axis=1)[:, :wi])
        np.save(os.path.join(seq, "depth", "%06d.npy" % i), d)
        np.save(os.path.join(seq, "normal", "%06d.npy" % i), nm)
        imgs.append(S.stack(d, nm, None, (True, True, False)))
    return np.stack(imgs)


def infer_end_to_end(tmp_path, fixture_npz, mcfg, h, wi, fw):
    """Infer with model section `mcfg` on five h x wi scans cut from the fixture images: overlap and yaw of every pair against the
    oracle, infer_top_k against decide_top_k on infer_multiple's outputs."""
    from overlapnet_amd import lcd
    from overlapnet_amd.infer import Infer
    n = 5
    imgs = _write_cues(str(tmp_path / "data"), fixture_npz, n, h, wi)
    cfg = {"model": mcfg, "infer_seqs": "07", "data_root_folder": str(tmp_path / "data"), "use_depth": True, "use_normals": True,
           "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16,
           "pretrained_weightsfilename": "", "precision": "f32"}
    w = S.make_test_weights(4, seed=0, model_cfg=mcfg, feat_w=fw)
    pairs = np.array([[i, j] for i in range(n) for j in range(n)])
    ov, yaw, _, corr, fv = O.infer_pairs(imgs, pairs, w, mcfg)
    ov, yaw, corr = ov.reshape(n, n), yaw.reshape(n, n), corr.reshape(n, n, fw)
    inf, tk = Infer(cfg, weights=w), Infer(cfg, weights=w)     # tk: infer_top_k, which caches each frame as infer_multiple does
    try:
        assert inf.feat_w == fw
        got_fv = inf.create_feature_volumes(["%06d" % i for i in range(n)])
        assert got_fv.shape == (n, 1, fw, 128)
        assert np.max(np.abs(got_fv - fv)) <= 2e-5 * np.max(np.abs(fv))
        assert inf.infer_multiple(0, []) is None               # caches frame 0 (a frame's cache index is its id)
        assert tk.infer_top_k(0, [], 3, None) == []
        for i in range(1, n):
            refs = list(range(i))
            o, y = inf.infer_multiple(i, refs)
            o, y = np.atleast_1d(o).copy(), np.atleast_1d(y).copy()
            for j in refs:
                assert abs(float(o[j]) - ov[j, i]) <= 1e-4, (i, j)
                if y[j] != yaw[j, i]:                              # a different bin only at a near-tie of the oracle's correlation
                    top = np.sort(corr[j, i])[::-1]
                    assert top[0] - top[1] <= 1e-5 * abs(top[0]), (i, j, y[j], yaw[j, i])
            k, thr = ((1, 0.3), (3, None), (5, 0.0), (2, 0.3))[i % 4]
            assert tk.infer_top_k(i, refs, k, thr) == lcd.decide_top_k(refs, o, y, k, thr), (i, k)
    finally:
        inf.close()
        tk.close()



@gpu
@pytest.mark.parametrize("fw", [45, 512], ids=lambda fw: "W%d" % fw)
def test_infer_end_to_end(tmp_path, fixture_npz, fw):
    """Infer on 32-beam scans of width 247 / 1181."""
    h, wi = WIDTHS[fw]
    infer_end_to_end(tmp_path, fixture_npz, _cfg(fw), h, wi, fw)
