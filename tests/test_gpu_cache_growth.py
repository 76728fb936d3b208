"""GPU (MI355X): the feature-volume cache of `Infer` through growth, overwrite, out-of-order slots and the look-ahead, on the real
engine (64 x 900 depth-only leg, feature width 360: the width that has spectra and Delta rows).
  a. the generated sequences of tests/_cache_model.py (what they reach is asserted on the CPU by tests/test_cache_growth_host.py) at
     min_capacity 2: every written slot's spectrum and Delta row, bit for bit, against one batched recomputation; and the batch
     independence that comparison rests on (a volume alone, in a batch of 64, in a batch of 65: both sides of the DFT launcher's switch);
  b. a 1-vs-N sweep over the grown cache: the bits of the sweep over a cache built in one piece with the volumes at the same slots,
     and of the scratch route; a sample of pairs against oracle/error_bounds, err / bound <= 1 (f16x3), as test_gpu_error_bounds.py;
  c. the shipped constant once: 1024 volumes, one more, 1024 -> 2050;
  d. `rebuild_delta_cache` on a grown cache after the head has been re-registered; the head registered A, B, A in every head precision;
  e. `Infer` over a run that grows its cache, with and without the look-ahead, against an `Infer` whose cache never grows;
  f. the slot sequence of one rank of a sharded `Infer`, without a process group.
Bits are compared as int32 words: a Delta row holds packed words that need not be numbers."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import error_bounds as E
from overlapnet_amd.infer import FeatureVolumeCache
from tools import synthetic as S

from tests import _cache_model as M

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

CFG = S.REFERENCE_MODEL_CFG
W1 = S.make_test_weights(1, seed=0)
FEAT_W, FEAT_C = 360, 128
_GROWN = {}


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    e = OvnEngine(64, 900, 1, device=0)
    e.load_weights(W1, CFG)
    assert e.feat_w == FEAT_W and e.has_spectrum and e.has_delta_cache
    yield e
    _GROWN.clear()
    e.close()


def _volumes(n, seed, dev):
    """n post-ReLU-like volumes made on the device: max(N(0.2, 1), 0), the distribution of oracle/error_bounds' plain volumes."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.clamp(torch.randn((n, FEAT_W, FEAT_C), generator=g, device=dev, dtype=torch.float32) + 0.2, min=0.0).contiguous()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


ROW_USED = FEAT_W * FEAT_C + 24 * 128 + 4      # csrc/delta_head_f16x3.hip: packed words | TT + b2 [24][128] | {max, min, 0, 0}


def _same_rows(a, b):
    """Delta cache rows: the words the kernels write and read.  The last 60 floats of a row (49216 = OVN_DELTA_CACHE_ELEMS) pad it
    to a multiple of 64; nothing writes them, so they hold whatever the allocation held."""
    assert a.shape[-1] == b.shape[-1] == 49216
    return _same_bits(a[..., :ROW_USED], b[..., :ROW_USED])


def _same_result(a, b, keys=("logit", "overlap", "yaw")):
    return all(_same_bits(a[k], b[k]) for k in keys)


def _grow_by_sequence(e, seed, min_capacity=2):
    ops, n_vols = M.generate_ops(seed, min_capacity)
    vols = _volumes(n_vols, 1000 + seed, e.device)
    cache, model = FeatureVolumeCache(e, min_capacity=min_capacity), M.CacheModel()
    log = M.run_ops(cache, model, ops, lambda j: vols[j])
    return cache, model, log


def _grown(e, seed):
    """The cache, model and log of sequence `seed` at min_capacity 2 on the shared engine, built once."""
    if seed not in _GROWN:
        _GROWN[seed] = _grow_by_sequence(e, seed)
    return _GROWN[seed]


def _held(model, dev):
    slots = model.slots()
    return slots, torch.tensor(slots, dtype=torch.int64, device=dev), torch.stack([model.vols[s] for s in slots])


# ---- a. the cache on the real engine ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", M.SEEDS)
def test_generated_sequences_on_the_real_engine(eng, seed):
    cache, model, log = _grown(eng, seed)
    causes = M.growth_causes(log)
    assert len(causes) >= 3 and set(M.GROWTH_CAUSES) <= set(causes) and M.overwrites_after_growth(log), causes
    slots, idx, vols = _held(model, eng.device)
    assert len(cache) == model.n and cache.shape == (model.n, 1, FEAT_W, FEAT_C)
    assert _same_bits(cache.device_features[idx], vols)
    assert _same_bits(cache.device_spectra[idx], eng.spectrum(vols)), "a cached spectrum is not its volume's"
    assert _same_rows(cache.device_delta_cache[idx], eng.delta_cache(vols)), "a cached Delta row is not its volume's"
    # the list view, copied from the device: the ends, a slice across a reallocation, the whole array
    arr = np.asarray(cache)
    assert arr.shape == (model.n, 1, FEAT_W, FEAT_C)
    assert np.array_equal(arr[slots], vols.cpu().numpy()[:, None])
    assert np.array_equal(cache[-1], model.vols[model.n - 1].cpu().numpy()[None])
    assert np.array_equal(cache[slots[0]], model.vols[slots[0]].cpu().numpy()[None])
    part = cache[1:6]
    assert len(part) == 5 and all(np.array_equal(part[s - 1], model.vols[s].cpu().numpy()[None]) for s in range(1, 6) if s in model.vols)
    with pytest.raises(IndexError):
        cache[model.n]


def test_spectrum_and_delta_row_do_not_depend_on_the_batch(eng):
    """A volume's spectrum / Delta row alone, in a batch of 64 and in a batch of 65: the same bits (the DFT launcher changes kernels
    at n <= 64, and the cache computes rows one frame at a time, k at a time and in whole-pool rebuilds)."""
    v = _volumes(65, 3, eng.device)
    for fn, same in ((eng.spectrum, _same_bits), (eng.delta_cache, _same_rows)):
        alone = {i: fn(v[i:i + 1]) for i in (0, 63, 64)}
        b64, b65 = fn(v[:64]), fn(v)
        assert same(b64[0:1], alone[0]) and same(b64[63:64], alone[63]), fn.__name__
        assert same(b65[:64], b64) and same(b65[64:65], alone[64]), fn.__name__


# ---- b. sweeps over the grown cache ----------------------------------------------------------------------------------------------
def _sweep(e, cache, q, qspec, lidx, dcache="cache", **kw):
    dc = cache.device_delta_cache if dcache == "cache" else dcache
    return e.heads(cache.device_features, q, lidx=lidx, n=len(lidx), spec_l=cache.device_spectra, spec_r=qspec, dcache_l=dc,
                   want_logit=True, **kw)


def _in_one_piece(e, model):
    """A cache that never reallocates, with the model's volumes at the model's slots (a pair's bits depend on the candidate's slot
    modulo 32) and zeros where nothing was written: one `extend_device` into an allocation of that size."""
    slots, idx, vols = _held(model, e.device)
    dense = torch.zeros((model.n, FEAT_W, FEAT_C), dtype=torch.float32, device=e.device)
    dense[idx] = vols
    fresh = FeatureVolumeCache(e, min_capacity=model.n)
    fresh.extend_device(dense)
    assert M.capacity(fresh) == model.n == len(fresh)
    return fresh


def test_sweep_over_the_grown_cache(eng):
    seed = M.SEEDS[0]
    cache, model, log = _grown(eng, seed)
    slots, idx, vols = _held(model, eng.device)
    assert len(M.growth_causes(log)) >= 3
    q = _volumes(1, 77, eng.device)
    qspec = eng.spectrum(q)
    lidx = np.asarray(slots, np.int32)
    grown = _sweep(eng, cache, q, qspec, lidx, want_corr=True)
    fresh = _sweep(eng, _in_one_piece(eng, model), q, qspec, lidx)
    scratch = _sweep(eng, cache, q, qspec, lidx, dcache=None)
    assert _same_result(grown, fresh), "the sweep over the grown cache differs from the sweep over a cache built in one piece"
    assert _same_result(grown, scratch), "cache rows and scratch preparation give different bits on the grown cache"
    # not only the code against itself: a sample of pairs against the fp64 statement and its bounds
    before, after, over = M.landmark_slots(log, model)
    assert before and after and over
    sample = []
    for s in [before[0], after[0], over[0], before[-1], after[-1], over[-1]] + slots[::-1]:
        if s not in sample and len(sample) < 8:
            sample.append(s)
    assert len(sample) >= 8 and set(sample) & set(before) and set(sample) & set(after) and set(sample) & set(over)
    qh = q[0].cpu().numpy()
    host = {s: model.vols[s].cpu().numpy() for s in sample}
    with ThreadPoolExecutor(8) as ex:
        oracle = list(ex.map(lambda s: (E.head_pair(host[s], qh, W1, 15), E.corr_pair(host[s], qh)), sample))
    lg, ov, corr = grown["logit"].cpu().numpy(), grown["overlap"].cpu().numpy(), grown["corr"].cpu().numpy()
    worst = {}
    for s, (h, c) in zip(sample, oracle):
        p = slots.index(s)
        B = E.head_bounds(h, W1, "f16x3")
        rat = {"logit": E.ratio(lg[p], h["logit"], B["logit"]), "overlap": E.ratio(ov[p], h["overlap"], B["overlap"]),
               "corr": E.ratio(corr[p], c["corr"], c["spectral"])}
        for k, v in rat.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("[grown cache, f16x3, slots %s] worst err / bound: %s" % (sample, {k: "%.3g" % v for k, v in sorted(worst.items())}))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, "over the bound: %s" % bad


# ---- c. the shipped constant -----------------------------------------------------------------------------------------------------
def test_the_default_capacity_grows_from_1024_to_2050(eng):
    vols = _volumes(1025, 5, eng.device)
    q = _volumes(1, 6, eng.device)
    qspec = eng.spectrum(q)
    a = b = None
    try:
        a = FeatureVolumeCache(eng)
        a.extend_device(vols[:1024])
        assert M.capacity(a) == 1024 and len(a) == 1024
        a.extend_device(vols[1024:])
        assert M.capacity(a) == 2050 and len(a) == 1025
        assert a._spec.shape[0] == 2050 and a._dc.shape[0] == 2050
        for i in (0, 1023, 1024):
            assert _same_bits(a.device_features[i:i + 1], vols[i:i + 1]), i
            assert _same_bits(a.device_spectra[i:i + 1], eng.spectrum(vols[i:i + 1])), i
            assert _same_rows(a.device_delta_cache[i:i + 1], eng.delta_cache(vols[i:i + 1])), i
        b = FeatureVolumeCache(eng)
        b.extend_device(vols)
        assert M.capacity(b) == 1025
        assert _same_bits(a.device_features, b.device_features)
        assert _same_bits(a.device_spectra, b.device_spectra) and _same_rows(a.device_delta_cache, b.device_delta_cache)
        ra = eng.heads(a.device_features, q, spec_l=a.device_spectra, spec_r=qspec, dcache_l=a.device_delta_cache, want_logit=True)
        rb = eng.heads(b.device_features, q, spec_l=b.device_spectra, spec_r=qspec, dcache_l=b.device_delta_cache, want_logit=True)
        assert ra["overlap"].shape[0] == 1025 and _same_result(ra, rb)
        torch.cuda.synchronize()
    finally:
        a = b = ra = rb = vols = None
        torch.cuda.empty_cache()


# ---- d. rebuild_delta_cache after growth -----------------------------------------------------------------------------------------
def test_rebuild_delta_cache_on_a_grown_cache_after_a_new_head():
    """The head is re-registered the way the trainers do it (`set_head_weights`; a finalized engine takes no second `load_weights`)."""
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 1, device=0)
    try:
        e.load_weights(W1, CFG)
        cache, model, log = _grow_by_sequence(e, M.SEEDS[1])
        assert len(M.growth_causes(log)) >= 3
        slots, idx, vols = _held(model, e.device)
        old_rows, old_spec = cache.device_delta_cache[idx].clone(), cache.device_spectra[idx].clone()
        assert _same_rows(old_rows, e.delta_cache(vols))
        w2 = S.make_test_weights(1, seed=5)
        e.set_head_weights([torch.from_numpy(np.ascontiguousarray(w2[k], np.float32)).to(e.device) for k in e.HEAD_PARAMS])
        cap = M.capacity(cache)
        cache.rebuild_delta_cache()
        assert M.capacity(cache) == cap and len(cache) == model.n
        rows = cache.device_delta_cache[idx]
        assert _same_rows(rows, e.delta_cache(vols)), "a rebuilt row is not its volume's under the new head"
        assert not _same_rows(rows, old_rows), "the second weight set must change the rows, or this test shows nothing"
        assert _same_bits(cache.device_features[idx], vols) and _same_bits(cache.device_spectra[idx], old_spec)
        q = _volumes(1, 78, e.device)
        qspec = e.spectrum(q)
        lidx = np.asarray(slots, np.int32)
        assert _same_result(_sweep(e, cache, q, qspec, lidx), _sweep(e, cache, q, qspec, lidx, dcache=None))
        torch.cuda.synchronize()
    finally:
        e.close()


def test_head_registered_again_and_again_in_every_precision():
    """Head weights A, then B, then A again, in each head precision: a 1-vs-6 sweep over Delta cache rows rebuilt after every
    registration and a 4-pair indexed call.  Under B the rows, logits and overlaps differ from those under A (the yaw head has no
    weights: its bins stay); after the second A everything is what it was after the first, bit for bit -- a device copy of the
    weight set that a registration leaves behind shows up as stale bits in one of the routes."""
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 1, device=0)
    try:
        e.load_weights(W1, CFG)
        sets = {name: [torch.from_numpy(np.ascontiguousarray(w[k], np.float32)).to(e.device) for k in e.HEAD_PARAMS]
                for name, w in (("A", W1), ("B", S.make_test_weights(1, seed=5)))}
        vols = _volumes(7, 79, e.device)
        cand, q = vols[:6], vols[6:7]
        spec = e.spectrum(vols)

        def run(precision):
            e.set_head_precision("f16x3")     # the engine builds rows in the modes that read them: the weight set decides them, not the mode
            rows = e.delta_cache(cand)
            e.set_head_precision(precision)
            sweep = e.heads(cand, q, spec_l=spec[:6], spec_r=spec[6:7], dcache_l=rows, want_logit=True)
            pairs = e.heads(vols, vols, lidx=[0, 1, 2, 3], ridx=[4, 5, 6, 2], spec_l=spec, spec_r=spec, want_logit=True)
            assert sweep["overlap"].shape[0] == 6 and pairs["overlap"].shape[0] == 4
            out = {"rows": rows[:, :ROW_USED]}
            for name, r in (("sweep", sweep), ("pairs", pairs)):
                out.update({"%s %s" % (name, k): r[k] for k in ("overlap", "logit", "yaw")})
            return out

        for precision in ("f16x3", "bf16x3", "f32"):
            got = []
            for name in "ABA":
                e.set_head_weights(sets[name])
                got.append(run(precision))
            first, other, again = got
            for k in first:
                assert _same_bits(again[k], first[k]), "%s: %s after the second registration of A is not what it was after the first" % (precision, k)
                if not k.endswith("yaw"):
                    assert not _same_bits(other[k], first[k]), "%s: %s is the same under both weight sets" % (precision, k)
        torch.cuda.synchronize()
    finally:
        e.close()


# ---- e. Infer over a run that grows ----------------------------------------------------------------------------------------------
N_FRAMES = 24


def _write_depth_sequence(root, fx, n):
    """n depth-only frames: frame i = fixture range image (i mod 2) rolled by 15 (i // 2) columns."""
    d = os.path.join(root, "07", "depth")
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        np.save(os.path.join(d, "%06d.npy" % i), np.ascontiguousarray(np.roll(fx["range_%d" % (i % 2)], 15 * (i // 2), axis=1)))


def _config(root, **extra):
    cfg = {"model": dict(CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(root), "use_depth": True,
           "use_normals": False, "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False,
           "batch_size": 16, "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


def _equal_answers(a, b):
    if a is None or b is None or isinstance(a, list):
        return a == b
    if isinstance(a, tuple) and isinstance(a[0], np.ndarray):          # infer_multiple: (overlap, yaw)
        return (np.array_equal(np.asarray(a[0]).view(np.int32), np.asarray(b[0]).view(np.int32))
                and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype)
    return a == b


def test_infer_over_a_growing_cache_with_and_without_the_look_ahead(tmp_path, fixture_npz, monkeypatch):
    """Every call of `infer_multiple` / `infer_top_k` / `infer_best_match` appends its frame, as the reference's list does: with the
    extra calls on every fourth and fifth frame the caches end at 35 volumes, and a capacity-2 cache reallocates at its 3rd, 7th,
    15th and 31st append.  The look-ahead frame of `infer_multiple(i)` is the one the previous call read ahead."""
    from overlapnet_amd.engine import QueryAhead
    from overlapnet_amd.infer import Infer
    root = str(tmp_path / "data")
    _write_depth_sequence(root, fixture_npz, N_FRAMES)
    A = Infer(_config(root, stream_ahead=True), weights=W1)
    B = Infer(_config(root, stream_ahead=True), weights=W1)
    C = Infer(_config(root, stream_ahead=False), weights=W1)
    taken = []
    take_all = QueryAhead.take_all

    def spy(self):
        taken.append(self)
        return take_all(self)
    monkeypatch.setattr(QueryAhead, "take_all", spy)
    try:
        A.feature_volumes = FeatureVolumeCache(A.engine, min_capacity=2)
        C.feature_volumes = FeatureVolumeCache(C.engine, min_capacity=2)
        assert M.capacity(A.feature_volumes) is None and isinstance(B.feature_volumes, FeatureVolumeCache)
        rng = np.random.default_rng(24)
        growths, adopted_by_the_growing_call, answers = 0, 0, 0

        def call(what, *args):
            nonlocal growths, adopted_by_the_growing_call, answers
            cap, n_taken = M.capacity(A.feature_volumes), sum(1 for t in taken if t is A._qa)
            ra = getattr(A, what)(*args)
            if cap is not None and M.capacity(A.feature_volumes) != cap:
                growths += 1          # one append per call: if this call adopted a look-ahead frame, that append grew the cache
                adopted_by_the_growing_call += int(sum(1 for t in taken if t is A._qa) > n_taken)
            rb, rc = getattr(B, what)(*args), getattr(C, what)(*args)
            assert _equal_answers(ra, rb), (what, args, ra, rb)
            assert _equal_answers(rc, rb), (what, args, rc, rb)
            answers += int(rb is not None and len(rb) > 0)

        for i in range(N_FRAMES):
            refs = list(range(i)) if i % 2 == 0 else sorted(int(r) for r in rng.choice(i, size=(i + 1) // 2, replace=False))
            call("infer_multiple", i, refs)
            if i % 4 == 0:
                call("infer_top_k", i, refs, 5, 0.0)
            if i % 5 == 0:
                call("infer_best_match", i, refs)
        assert answers >= N_FRAMES
        n = len(A.feature_volumes)
        assert n == N_FRAMES + len(range(0, N_FRAMES, 4)) + len(range(0, N_FRAMES, 5)) == len(B.feature_volumes) == len(C.feature_volumes)
        assert growths >= 3 and M.capacity(B.feature_volumes) == 1024 and M.capacity(C.feature_volumes) == M.capacity(A.feature_volumes)
        assert adopted_by_the_growing_call >= 1, "no look-ahead frame was appended by a call that grew the cache"
        assert C._qa is None and any(t is B._qa for t in taken)
        fb = B.feature_volumes
        for other in (A.feature_volumes, C.feature_volumes):
            assert _same_bits(other.device_features, fb.device_features)
            assert _same_bits(other.device_spectra, fb.device_spectra)
            assert _same_rows(other.device_delta_cache, fb.device_delta_cache)
        # the reference's way to reset the cache, on a grown one
        A.feature_volumes = []
        B.feature_volumes = []
        assert len(A.feature_volumes) == 0 and M.capacity(A.feature_volumes) is None
        for i in range(3):
            ra, rb = A.infer_multiple(i, list(range(i))), B.infer_multiple(i, list(range(i)))
            assert _equal_answers(ra, rb), (i, ra, rb)
        assert len(A.feature_volumes) == 3 and _same_bits(A.feature_volumes.device_features, B.feature_volumes.device_features)
        assert _same_bits(A.feature_volumes.device_features, fb.device_features[[0, 3, 4]])       # frames 0, 1, 2 of the first run
        # ... and the reference's other assignment: a list of host volumes rebuilds the device cache, spectra and rows included
        A.feature_volumes = list(B.feature_volumes)
        fa, fb = A.feature_volumes, B.feature_volumes
        assert len(fa) == 3 and _same_bits(fa.device_features, fb.device_features)
        assert _same_bits(fa.device_spectra, fb.device_spectra) and _same_rows(fa.device_delta_cache, fb.device_delta_cache)
        assert _equal_answers(A.infer_multiple(3, [0, 1, 2]), B.infer_multiple(3, [0, 1, 2]))
        torch.cuda.synchronize()
    finally:
        for inf in (A, B, C):
            inf.close()


# ---- f. sharded slots without a process group ------------------------------------------------------------------------------------
def test_sharded_slot_sequence_on_the_real_engine(eng):
    n_frames = 40
    seq = M.sharded_slots(n_frames, 1, 4)
    frames, slots = [f for f, _ in seq], [s for _, s in seq]
    assert any(b < a for a, b in zip(slots, slots[1:])) and all(s % 32 == f % 32 for f, s in seq)
    vols = _volumes(n_frames, 9, eng.device)
    cache = FeatureVolumeCache(eng, min_capacity=2)
    growths = 0
    for f, s in seq:
        cap = M.capacity(cache)
        cache.put_device(s, vols[f:f + 1])
        growths += int(cap is not None and M.capacity(cache) != cap)
    assert growths >= 3 and len(cache) == max(slots) + 1
    idx = torch.tensor(slots, dtype=torch.int64, device=eng.device)
    assert _same_bits(cache.device_features[idx], vols[frames])
    whole = FeatureVolumeCache(eng, min_capacity=n_frames)
    whole.extend_device(vols)
    assert M.capacity(whole) == n_frames
    assert _same_bits(cache.device_spectra[idx], whole.device_spectra[frames])
    assert _same_rows(cache.device_delta_cache[idx], whole.device_delta_cache[frames])
    q = _volumes(1, 10, eng.device)
    qspec = eng.spectrum(q)
    sharded = _sweep(eng, cache, q, qspec, np.asarray(slots, np.int32))
    unsharded = _sweep(eng, whole, q, qspec, np.asarray(frames, np.int32))
    assert _same_result(sharded, unsharded), "the owned frames at their slots do not give the unsharded sweep's bits"
