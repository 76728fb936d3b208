"""CPU: `FeatureVolumeCache` (overlapnet_amd/infer.py) through growth, overwrite, out-of-order slots and scattered writes, side by
side with its plain statement (tests/_cache_model.py), on a fake engine whose "spectrum" and "Delta row" are injective functions of
the volume (and, for the row, of the registered head): a row then names the volume it was computed from, and a stale, shifted or
dropped row after a reallocation shows.  The sequences are generated; what each of them reaches (how many reallocations, caused by
which operation, an overwrite afterwards) is asserted here, so the GPU test that replays them inherits the reach."""
import numpy as np
import pytest
import torch

from overlapnet_amd.infer import FeatureVolumeCache

from tests import _cache_model as M

FEAT_C = 128
W = 6            # a small feature width: the cache takes the engine's, and nothing here depends on 360


class FakeEngine(object):
    """What `FeatureVolumeCache` needs of its engine, on the CPU."""
    SPEC_W = 5
    DELTA_CACHE_ELEMS = 11

    def __init__(self, has_spectrum=True, has_delta_cache=True, feat_w=W):
        self.device = torch.device("cpu")
        self.has_spectrum = has_spectrum
        self.has_delta_cache = has_delta_cache
        self.feat_w = feat_w
        self.head_version = 0
        self.calls = {"spectrum": 0, "delta_cache": 0}

    def spectrum(self, fv, out=None):
        assert self.has_spectrum and fv.dtype == torch.float32 and tuple(fv.shape[1:]) == (self.feat_w, FEAT_C)
        self.calls["spectrum"] += 1
        r = spec_of(fv)
        if out is None:
            return r
        assert tuple(out.shape) == tuple(r.shape) and out.is_contiguous()
        out.copy_(r)
        return out

    def delta_cache(self, fv, out=None):
        assert self.has_delta_cache and fv.dtype == torch.float32 and tuple(fv.shape[1:]) == (self.feat_w, FEAT_C)
        self.calls["delta_cache"] += 1
        r = row_of(fv, self.head_version)
        if out is None:
            return r
        assert tuple(out.shape) == tuple(r.shape) and out.is_contiguous()
        out.copy_(r)
        return out


def spec_of(fv):
    """(n, W, 128) -> (n, 128, SPEC_W): the first 128 x SPEC_W values of each volume times 3."""
    n = fv.shape[0]
    return (3.0 * fv.reshape(n, -1)[:, :FEAT_C * FakeEngine.SPEC_W]).reshape(n, FEAT_C, FakeEngine.SPEC_W)


def row_of(fv, version):
    """(n, W, 128) -> (n, DELTA_CACHE_ELEMS): the volume's first values times -7, plus the head version."""
    n = fv.shape[0]
    return -7.0 * fv.reshape(n, -1)[:, :FakeEngine.DELTA_CACHE_ELEMS] + float(version)


def _volumes(n, seed):
    """n distinct volumes of small integers (every product above is exact): the first values of volume i spell i."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 50, size=(n, W, FEAT_C)).astype(np.float32)
    v[:, 0, 0] = np.arange(n)
    return torch.from_numpy(v)


def _check_pools(cache, model, eng, spectral, with_dc):
    assert len(cache) == model.n
    assert cache.shape == (model.n, 1, W, FEAT_C)
    feats, spec, dc = cache.device_features, cache.device_spectra, cache.device_delta_cache
    assert tuple(feats.shape) == (model.n, W, FEAT_C)
    assert (spec is None) == (not spectral) and (dc is None) == (not with_dc)
    if spectral:
        assert tuple(spec.shape) == (model.n, FEAT_C, eng.SPEC_W)
    if with_dc:
        assert tuple(dc.shape) == (model.n, eng.DELTA_CACHE_ELEMS)
    for s in model.slots():
        v = model.vols[s]
        assert torch.equal(feats[s], v), "slot %d holds another volume (its first value: %g, wanted %g)" % (s, feats[s, 0, 0], v[0, 0])
        if spectral:
            assert torch.equal(spec[s], spec_of(v[None])[0]), "slot %d: the spectrum is not this volume's" % s
        if with_dc:
            assert torch.equal(dc[s], row_of(v[None], model.stamp[s])[0]), "slot %d: the Delta row is not this volume's / this head's" % s


def _check_list_behaviour(cache, model):
    """`len()`, `[i]`, negative indices, slices, iteration and `np.asarray` against the model (written slots only: a slot below the
    high-water mark that no frame has reached yet holds nothing anyone may refer to)."""
    n = model.n
    held = model.slots()
    arr = np.asarray(cache)
    assert arr.shape == (n, 1, W, FEAT_C) and arr.dtype == np.float32
    items = list(cache)
    assert len(items) == n
    for s in held:
        want = model.vols[s].numpy().reshape(1, W, FEAT_C)
        for got in (cache[s], cache[s - n], items[s], arr[s]):
            assert got.shape == (1, W, FEAT_C) and np.array_equal(got, want), s
    assert np.array_equal(cache[-1], model.vols[n - 1].numpy()[None])           # the highest slot is always a written one
    for a, b in ((0, n), (1, n - 1), (n // 2, None), (-3, None), (None, 2), (n, n + 5), (0, 0)):
        got, want = cache[a:b], list(range(n))[a:b]
        assert len(got) == len(want)
        for g, s in zip(got, want):
            if s in model.vols:
                assert np.array_equal(g, model.vols[s].numpy()[None]), (a, b, s)
    for bad in (n, n + 3, -n - 1):
        with pytest.raises(IndexError):
            cache[bad]
    assert np.asarray(cache, dtype=np.float64).dtype == np.float64


CONFIGS = {
    "spectra+rows": dict(has_spectrum=True, has_delta_cache=True, with_delta_cache=True),
    "width!=360": dict(has_spectrum=False, has_delta_cache=False, with_delta_cache=True),          # no spectra, no rows
    "conv1size!=15": dict(has_spectrum=True, has_delta_cache=False, with_delta_cache=True),        # spectra, no rows
    "throw-away": dict(has_spectrum=True, has_delta_cache=True, with_delta_cache=False),           # rows not wanted
}


def _run(seed, min_capacity, cfg):
    eng = FakeEngine(cfg["has_spectrum"], cfg["has_delta_cache"])
    cache = FeatureVolumeCache(eng, min_capacity=min_capacity, with_delta_cache=cfg["with_delta_cache"])
    model = M.CacheModel()
    ops, n_vols = M.generate_ops(seed, min_capacity)
    vols = _volumes(n_vols, seed)
    spectral, with_dc = cfg["has_spectrum"], cfg["has_delta_cache"] and cfg["with_delta_cache"]
    cap = [None]

    def reregister():                      # a trainer re-registers the head, then asks for the rows again
        eng.head_version += 1
        model.head_version += 1

    def after(e):
        need = e["n_after"]
        cap[0] = M.predicted_capacity(cap[0], need, min_capacity)
        assert e["cap_after"] == cap[0], (e, cap[0])                       # the allocation rule: need, then 2 x need
        for pool, on in ((cache._spec, spectral), (cache._dc, with_dc)):
            assert pool.shape[0] == (e["cap_after"] if on else 0)
        _check_pools(cache, model, eng, spectral, with_dc)
        _check_list_behaviour(cache, model)

    assert len(cache) == 0 and list(cache) == [] and np.asarray(cache).shape == (0, 1, W, FEAT_C) and cache[0:3] == []
    assert tuple(cache.device_features.shape) == (0, W, FEAT_C)
    with pytest.raises(IndexError):
        cache[0]
    log = M.run_ops(cache, model, ops, lambda j: vols[j], after=after, before_rebuild=reregister)
    return log, cache, model, eng


@pytest.mark.parametrize("min_capacity", [1, 2, 7])
@pytest.mark.parametrize("seed", M.SEEDS)
def test_generated_sequences_reach_what_they_are_there_for(seed, min_capacity):
    """Conditions on the INPUTS (observed on the real class): every sequence reallocates at least three times, once at least through
    each of extend_device, put_device beyond the end, put_slots_device and append, and overwrites below the end afterwards."""
    log, cache, model, eng = _run(seed, min_capacity, CONFIGS["spectra+rows"])
    causes = M.growth_causes(log)
    assert len(causes) >= 3, causes
    for kind in M.GROWTH_CAUSES:
        assert kind in causes, (kind, causes)
    assert M.overwrites_after_growth(log)
    assert log[0]["cap_before"] is None and log[0]["cap_after"] == max(min_capacity, log[0]["n_after"])
    assert any(e["kind"] == "rebuild" and e["i"] > min(x["i"] for x in log if x["grew"]) for e in log)     # a rebuild on a grown cache
    before, after, over = M.landmark_slots(log, model)
    assert before and after and over
    holes = set(range(model.n)) - set(model.vols)
    assert holes, "a write beyond the end must leave unwritten slots below the high-water mark"


@pytest.mark.parametrize("name", sorted(CONFIGS))
@pytest.mark.parametrize("min_capacity", [1, 2, 7])
@pytest.mark.parametrize("seed", M.SEEDS)
def test_cache_follows_the_model_through_growth(seed, min_capacity, name):
    """Every check runs after every operation (`after` in `_run`); here the end state once more, and what the configuration means
    for the engine: no spectrum / row is ever asked of an engine that has none."""
    cfg = CONFIGS[name]
    log, cache, model, eng = _run(seed, min_capacity, cfg)
    assert len(M.growth_causes(log)) >= 3
    assert (eng.calls["spectrum"] > 0) == cfg["has_spectrum"]
    assert (eng.calls["delta_cache"] > 0) == (cfg["has_delta_cache"] and cfg["with_delta_cache"])


@pytest.mark.parametrize("min_capacity", [1, 2, 7])
def test_rows_handed_in_by_the_caller_survive_growth(min_capacity):
    """The streaming path: `extend_device(fv, spec=, dc=)` with rows computed elsewhere (QueryAhead), one frame per call.  The cache
    must keep exactly those rows -- marked here so that they differ from what the engine would compute -- across every reallocation."""
    eng = FakeEngine()
    cache = FeatureVolumeCache(eng, min_capacity=min_capacity)
    vols = _volumes(40, 5)
    grew = 0
    for i in range(40):
        cap = M.capacity(cache)
        cache.extend_device(vols[i:i + 1], spec=spec_of(vols[i:i + 1]) + 0.5, dc=row_of(vols[i:i + 1], 0) + 0.25)
        grew += int(cap is not None and M.capacity(cache) != cap)
        assert len(cache) == i + 1
        assert torch.equal(cache.device_features, vols[:i + 1])
        assert torch.equal(cache.device_spectra, spec_of(vols[:i + 1]) + 0.5)
        assert torch.equal(cache.device_delta_cache, row_of(vols[:i + 1], 0) + 0.25)
    assert grew >= 3 and eng.calls == {"spectrum": 0, "delta_cache": 0}
    eng.head_version = 3
    cache.rebuild_delta_cache()
    assert torch.equal(cache.device_delta_cache, row_of(vols, 3)) and torch.equal(cache.device_spectra, spec_of(vols) + 0.5)


def test_sharded_slot_sequence_of_rank_1_of_4():
    """200 frames, rank 1 of 4: the frames it owns arrive out of slot order, each through `put_device` at its slot, as
    `Infer._query_frame_sharded` writes them.  After every reallocation, and at the end, every owned frame is at its slot."""
    seq = M.sharded_slots(200, 1, 4)
    frames, slots = [f for f, _ in seq], [s for _, s in seq]
    assert len(seq) == 50 and len(set(slots)) == len(slots)
    assert all(s % 32 == f % 32 for f, s in seq)
    assert any(b < a for a, b in zip(slots, slots[1:])), "the slots must not arrive in increasing order"
    assert slots[0] > 0, "the first owned frame lands beyond the end of an empty cache"
    eng = FakeEngine()
    cache = FeatureVolumeCache(eng, min_capacity=2)
    model = M.CacheModel()
    vols = _volumes(200, 9)
    growths = 0
    for f, s in seq:
        cap = M.capacity(cache)
        cache.put_device(s, vols[f:f + 1])
        model.put(s, [vols[f]])
        if cap is not None and M.capacity(cache) != cap:
            growths += 1
            _check_pools(cache, model, eng, True, True)
        assert len(cache) == model.n == max(slots[:frames.index(f) + 1]) + 1
    assert growths >= 3
    _check_pools(cache, model, eng, True, True)
    _check_list_behaviour(cache, model)
    assert [int(cache.device_features[s, 0, 0]) for s in slots] == frames          # the volume at a frame's slot spells the frame id


def test_refusals_leave_the_cache_as_it_was():
    eng = FakeEngine()
    cache = FeatureVolumeCache(eng, min_capacity=2)
    model = M.CacheModel()
    vols = _volumes(12, 1)
    cache.extend_device(vols[:5])
    model.extend(list(vols[:5]))
    cap = M.capacity(cache)
    for slots, fv in (([1, 1], vols[5:7]),            # duplicate slots
                      ([9, 2, 9], vols[5:8]),
                      ([-1, 2], vols[5:7]),           # a negative slot
                      ([0, 1, 2], vols[5:7]),         # more slots than volumes
                      ([40], vols[5:7])):             # fewer (and one that would have grown the pools)
        with pytest.raises(ValueError):
            cache.put_slots_device(slots, fv)
        assert M.capacity(cache) == cap
        _check_pools(cache, model, eng, True, True)
    cache.put_slots_device([], vols[:0])              # nothing to write: not an error, nothing changes
    _check_pools(cache, model, eng, True, True)
    for bad in (5, 6, -6, 1 << 40):
        with pytest.raises(IndexError):
            cache[bad]
    assert cache[5:9] == [] and len(cache[-2:]) == 2
    with pytest.raises(Exception):
        cache.append(np.zeros((1, W + 1, FEAT_C), np.float32))       # a volume of another width
    _check_pools(cache, model, eng, True, True)
