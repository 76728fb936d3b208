"""GPU (MI355X): batches of loop-closure queries, each with its own candidate list, in one pass (`ovn_heads_segments`,
`ovn_top_k_segments`, the `Infer.*_batch` methods and `lcd.detect_offline`).  The rule is strict: every pair gets exactly the bits of
the per-query 1-vs-N loop, and every segment's records exactly those of `top_k` / `best_match` on its slice.
  * the engine in f16x3 at W = 360 on both routes (segmented passes with compaction on, the indexed pass with it off), passes that
    cut segments (a small head chunk), Delta cache rows on and off, packed last slices and a query with a negative value; bf16x3, f32
    and W = 371;
  * the f16x3 batch against the fp64 oracle's elementwise bound;
  * the segmented top-k against `top_k` per segment with ties, +-0, NaN, empty segments, and k = 1 against `best_match`;
  * `Infer` replaying the demo3 transcript against a second object that caches the frames and runs the batch methods."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd import lcd
from overlapnet_amd.engine import OvnEngine
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = S.REFERENCE_MODEL_CFG


@pytest.fixture(scope="module")
def eng():
    torch.cuda.set_device(0)
    e = OvnEngine(64, 900, 4, device=0)
    e.load_weights(S.make_trained_like_weights(4), CFG)
    yield e
    e.close()


def _pool(seed=5, k=24):
    """k volumes with varied live-channel lists: 32 random dead channels each, queries whose live channels end in packed last
    slices of 1 / 4 / 16 channels (97 / 100 / 112 live), one all-live, one with a negative value (no cache rows for its pairs)."""
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.2, 1.0, size=(k, 360, 128)), 0).astype(np.float32)
    for i in range(6, k):
        v[i][:, rng.permutation(128)[:32]] = 0
    for i, live in ((0, 97), (1, 100), (2, 112)):
        v[i][:, live:] = 0
    v[4, 17, 5] = -0.25
    return v


def _segments(rng, npool, nq, qoff=0):
    """(seg_offsets, query_idx, cand_idx): empty, 1, 3, 17, a segment longer than the test's head chunk, repeated candidates, a
    query that is also one of its own candidates (query pool = pool[qoff:]), and empty segments at both ends."""
    lens = [0, 1, 3, 17, 150, 0, 5, 40, 2, 0]
    q = rng.integers(0, nq, len(lens)).astype(np.int32)
    cands = []
    for b, n in enumerate(lens):
        c = rng.integers(0, npool, n).astype(np.int32)
        if n >= 3:
            c[1] = c[0]                    # a repeated candidate
            c[2] = q[b] + qoff             # the query against itself
        cands.append(c)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offs, q, np.concatenate(cands)


def _per_query(e, pool, qpool, offs, q, cand, spec, qspec, dc, corr=True):
    """The reference: each segment alone, in its 1-vs-N form (`heads` with lidx and the query as the right-hand volume)."""
    outs = []
    for b in range(len(q)):
        o0, o1 = int(offs[b]), int(offs[b + 1])
        if o0 == o1:
            continue
        qi = int(q[b])
        kw = {}
        if spec is not None:
            kw = dict(spec_l=spec, spec_r=qspec[qi:qi + 1], dcache_l=dc)
        outs.append(e.heads(pool, qpool[qi:qi + 1], lidx=cand[o0:o1], want_logit=True, want_corr=corr, **kw))
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}


def _equal(a, b, what):
    for k in ("overlap", "yaw", "logit", "corr"):
        if k in b:
            assert torch.equal(a[k], b[k]), (what, k)


def test_f16x3_batch_is_the_per_query_loop_bit_for_bit(eng):
    v = _pool()
    pool = torch.from_numpy(v).cuda()
    qpool = pool[3:].contiguous()          # a separate query pool (its own indexing)
    spec, qspec, dc = eng.spectrum(pool), eng.spectrum(qpool), eng.delta_cache(pool)
    rng = np.random.default_rng(11)
    assert eng.head_precision == "f16x3"
    try:
        for trial, comp in ((0, True), (1, True), (2, False)):
            # compaction on: segmented passes (one kernel chain per pass, query state per segment); off: one indexed pass
            eng.set_head_compaction(comp)
            offs, q, cand = _segments(rng, len(v), qpool.shape[0], qoff=3)
            for with_dc in (dc, None):
                want = _per_query(eng, pool, qpool, offs, q, cand, spec, qspec, with_dc)
                # chunk 1024: every segment in one pass; 64 and 7: passes that cut segments (the 150-pair one several times)
                for chunk in (1024, 64, 7):
                    eng.set_head_pipeline(chunk)
                    got = eng.heads_segments(pool, qpool, cand, q, offs, spec_pool=spec, spec_q=qspec, dcache_pool=with_dc,
                                             want_logit=True, want_corr=True)
                    _equal(got, want, (trial, chunk, with_dc is not None))
                eng.set_head_pipeline()
            # without spectra: the direct yaw head, ovn_heads' bits
            want = _per_query(eng, pool, qpool, offs, q, cand, None, None, None)
            got = eng.heads_segments(pool, qpool, torch.from_numpy(cand).cuda(), q, offs, want_logit=True, want_corr=True)
            _equal(got, want, (trial, "direct"))
    finally:
        eng.set_head_compaction(True)
        eng.set_head_pipeline()
    # the same pool as queries (Infer's cache), a device cand_idx, and the degenerate batches
    offs = np.array([0, 3, 3, 8], np.int64)
    q = np.array([2, 0, 7], np.int32)
    cand = torch.tensor([1, 2, 9, 0, 0, 5, 7, 7], dtype=torch.int32, device="cuda")
    got = eng.heads_segments(pool, pool, cand, q, offs, spec_pool=spec, spec_q=spec, dcache_pool=dc, want_logit=True)
    want = _per_query(eng, pool, pool, offs, q, cand.cpu().numpy(), spec, spec, dc, corr=False)
    _equal(got, want, "shared pool")
    assert eng.heads_segments(pool, pool, [], [0, 1], [0, 0, 0])["overlap"].shape == (0,)
    assert eng.heads_segments(pool, pool, [], [], [0])["yaw"].shape == (0,)


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_other_modes_batch_is_the_per_query_loop(eng, mode):
    v = _pool(seed=9, k=20)
    pool = torch.from_numpy(v).cuda()
    rng = np.random.default_rng(3)
    offs, q, cand = _segments(rng, len(v), len(v))
    eng.set_head_precision(mode)
    try:
        spec = eng.spectrum(pool)
        want = _per_query(eng, pool, pool, offs, q, cand, spec, spec, None)
        got = eng.heads_segments(pool, pool, cand, q, offs, spec_pool=spec, spec_q=spec, want_logit=True, want_corr=True)
        _equal(got, want, mode)
    finally:
        eng.set_head_precision("f16x3")


def test_width_371_batch_is_the_per_query_loop():
    cfg = dict(CFG, inputShape=[32, 900], leg_output_width=371, additional_unsymmetric_layer3a=False)
    e = OvnEngine(32, 900, 4)
    try:
        e.load_weights(S.make_test_weights(4, seed=0, model_cfg=cfg, feat_w=371), cfg)
        assert e.feat_w == 371
        rng = np.random.default_rng(8)
        v = np.maximum(rng.normal(0.2, 1.0, size=(12, 371, 128)), 0).astype(np.float32)
        pool = torch.from_numpy(v).cuda()
        offs, q, cand = _segments(rng, len(v), len(v))
        for mode in ("f16x3", "f32"):
            e.set_head_precision(mode)
            want = _per_query(e, pool, pool, offs, q, cand, None, None, None)
            got = e.heads_segments(pool, pool, cand, q, offs, want_logit=True, want_corr=True)
            _equal(got, want, ("371", mode))
    finally:
        e.close()


def test_f16x3_batch_against_the_fp64_bound():
    w = S.make_test_weights(4, seed=0)
    e = OvnEngine(64, 900, 4)
    try:
        e.load_weights(w, CFG)
        sets = E.value_edge_sets()
        name = sorted(sets)[0]
        v = np.ascontiguousarray(sets[name])
        k = v.shape[0]
        fv = torch.from_numpy(v).cuda()
        spec, dc = e.spectrum(fv), e.delta_cache(fv)
        # every volume a query once: against all of them, or against the first few
        q = np.arange(k, dtype=np.int32)
        cand = np.concatenate([np.arange(k) if b % 2 == 0 else np.arange(min(b, k)) for b in range(k)]).astype(np.int32)
        offs = np.concatenate([[0], np.cumsum([k if b % 2 == 0 else min(b, k) for b in range(k)])]).astype(np.int64)
        r = e.heads_segments(fv, fv, cand, q, offs, spec_pool=spec, spec_q=spec, dcache_pool=dc, want_logit=True, want_corr=True)
        lg, ov, corr = r["logit"].cpu().numpy(), r["overlap"].cpu().numpy(), r["corr"].cpu().numpy()
        worst = {}
        for b in range(k):
            for p in range(int(offs[b]), int(offs[b + 1])):
                h, c = E.head_pair(v[cand[p]], v[q[b]], w, 15), E.corr_pair(v[cand[p]], v[q[b]])
                B = E.head_bounds(h, w, "f16x3")
                for key, val in (("logit", E.ratio(lg[p], h["logit"], B["logit"])), ("overlap", E.ratio(ov[p], h["overlap"], B["overlap"])),
                                 ("corr", E.ratio(corr[p], c["corr"], c["spectral"]))):
                    worst[key] = max(worst.get(key, 0.0), val)
        print("[batch %s f16x3] worst err / bound: %s" % (name, {kk: "%.3g" % vv for kk, vv in sorted(worst.items())}))
        assert all(vv <= 1.0 for vv in worst.values()), worst
    finally:
        e.close()


def _scores(rng, n):
    v = (rng.integers(0, 12, n) / 12.0).astype(np.float32)        # heavy ties
    pick = rng.random(n)
    v[pick < 0.1] = np.nan
    v[(pick >= 0.1) & (pick < 0.2)] = 0.0
    v[(pick >= 0.2) & (pick < 0.3)] = -0.0
    return v


def test_top_k_segments_is_top_k_per_segment(eng):
    rng = np.random.default_rng(21)
    lens = [0, 1, 5, 1024, 0, 3000, 7, 2, 1500, 0]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1])
    ov = torch.from_numpy(_scores(rng, n)).cuda()
    yaw = torch.from_numpy(rng.integers(-179, 181, n).astype(np.int32)).cuda()
    ids = torch.from_numpy(rng.integers(0, 1 << 20, n).astype(np.int32)).cuda()
    for k in (1, 5, 1024):
        for y, i in ((yaw, ids), (None, None)):
            got = eng.top_k_segments(ov, offs, y, k, 0.5, ids=i)
            assert got.shape == (len(lens), k, 4)
            for b in range(len(lens)):
                o0, o1 = int(offs[b]), int(offs[b + 1])
                want = eng.top_k(ov[o0:o1].contiguous(), None if y is None else y[o0:o1].contiguous(), k, 0.5,
                                 ids=None if i is None else i[o0:o1].contiguous())
                assert torch.equal(got[b], want), (k, b)
                if o0 == o1:
                    assert got[b].tolist() == [[-1, 0, 0, 0]] * k
                if k == 1:
                    m = eng.best_match(ov[o0:o1].contiguous(), None if y is None else y[o0:o1].contiguous(), 0.5,
                                       ids=None if i is None else i[o0:o1].contiguous())
                    assert torch.equal(got[b, 0], m), b
    assert eng.top_k_segments(ov[:0], [0], k=3).shape == (0, 3, 4)


# ---- through Infer -----------------------------------------------------------------------------------------------------------------
def _write_sequence(root, fx, n):
    """n frames: frame i = fixture scan (i mod 2) rolled by 40 (i // 2) columns."""
    seq = os.path.join(root, "07")
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(seq, sub), exist_ok=True)
    for i in range(n):
        s, shift = i % 2, (40 * (i // 2)) % 900
        np.save(os.path.join(seq, "depth", "%06d.npy" % i), np.ascontiguousarray(np.roll(fx["range_%d" % s], shift, axis=1)))
        np.save(os.path.join(seq, "normal", "%06d.npy" % i), np.ascontiguousarray(np.roll(fx["normal_%d" % s], shift, axis=1)))


def _config(root):
    return {"model": dict(CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(root), "use_depth": True,
            "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False,
            "batch_size": 16, "pretrained_weightsfilename": ""}


def _transcript_calls():
    with open(os.path.join(ROOT, "tests", "golden", "demo_transcript.json")) as f:
        d = json.load(f)
    return [(int(c["cur"]), [int(r) for r in c["refs"]]) for c in d["demo3"] if c.get("event") == "infer_multiple"]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, tuple) and isinstance(a[0], np.ndarray):
        return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))
    return a == b


def test_infer_batch_methods_replay_the_demo3_transcript(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    calls = _transcript_calls()
    assert len(calls) == 259 and [c for c, _ in calls] == list(range(259))
    _write_sequence(str(tmp_path / "data"), fixture_npz, 259)
    w = S.make_test_weights(4, seed=0)
    a, b = Infer(_config(tmp_path / "data"), weights=w), Infer(_config(tmp_path / "data"), weights=w)
    try:
        want_multi, want_best, nonempty = [], {}, 0
        for cur, refs in calls:
            if refs:
                nonempty += 1
                if nonempty % 7 == 0:
                    want_best[cur] = a.infer_best_match(cur, refs, 0.3)
                    want_multi.append(None)
                    continue
            want_multi.append(a.infer_multiple(cur, refs))
        assert nonempty == 83
        b.cache_frames(259)
        assert len(b.feature_volumes) == 259
        assert torch.equal(a.feature_volumes.device_features, b.feature_volumes.device_features)
        cur_ids = [c for c, _ in calls]
        lists = [r for _, r in calls]
        got_multi = b.infer_multiple_batch(cur_ids, lists)
        for (cur, refs), g, wnt in zip(calls, got_multi, want_multi):
            if cur in want_best:
                continue
            assert _same(g, wnt), cur
        got_best = b.infer_best_match_batch(cur_ids, lists, 0.3)
        for cur, m in want_best.items():
            assert got_best[cur] == m, cur
        got_top = b.infer_top_k_batch(cur_ids, lists, 5, None)
        for (cur, refs), g, res in zip(calls, got_top, got_multi):
            assert g == ([] if res is None else lcd.decide_top_k(refs, res[0], res[1], 5, None)), cur
            m = got_best[cur]
            assert b.infer_top_k_batch([cur], [refs], 1, 0.3)[0] == ([m] if m else []), cur
        with pytest.raises(IndexError):
            b.infer_multiple_batch([259], [[0]])
    finally:
        a.close()
        b.close()


def test_detect_offline_equals_the_detect_loop(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    n = 140
    _write_sequence(str(tmp_path / "data"), fixture_npz, n)
    rng = np.random.default_rng(4)
    xy = np.cumsum(rng.normal(0, 1.0, size=(n, 2)), axis=0)
    xy[110:] = xy[:30] + rng.normal(0, 0.5, size=(30, 2))          # a loop back to the start
    length = lcd.travelled_distances(xy)
    ell = lcd.covariance_ellipse(np.eye(2) * 4.0)
    w = S.make_test_weights(4, seed=0)
    a, b = Infer(_config(tmp_path / "data"), weights=w), Infer(_config(tmp_path / "data"), weights=w)
    try:
        kw = dict(inactive_time_thres=100, inactive_dist_thres=5.0, overlap_thres=0.2)
        loop = [lcd.detect(a, i, xy, length, ell, **dict(kw)) for i in range(n)]
        got = lcd.detect_offline(b, range(n), xy, length, ell, **dict(kw))
        assert got == loop
        assert sum(len(lcd.gate_candidates(i, xy, length, ell, 100, 5.0)) > 0 for i in range(n)) > 0
    finally:
        a.close()
        b.close()
