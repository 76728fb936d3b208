"""GPU (MI355X): the top-k loop-closure candidates, ranked on the device (`ovn_top_k`, csrc/top_k.hip).
  * `OvnEngine.top_k` against the host statement of its order (`lcd.decide_top_k`), record by record and bit for bit, over sizes
    around k and the workgroup width up to 2^20 + 7, on all-equal arrays, heavy ties, NaN runs, +-0, +-inf and subnormals, with and
    without yaw / ids / index_offset; k = 1 against `best_match`; two calls against each other; the argument refusals;
  * `Infer.infer_top_k` on the real heads against `decide_top_k` on `infer_multiple`'s outputs of an identical object, the k = 1
    invariant with `infer_best_match`, threshold filtering / None / the empty list, and one run at a leg output width of 371."""
import os

import numpy as np
import pytest
import torch

from overlapnet_amd import lcd
from overlapnet_amd._lib import OvnError
from overlapnet_amd.engine import OvnEngine, decode_top_k
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

KS = (1, 2, 7, 64, 1000, 1024)
KINDS = ("equal", "ties", "nan_runs", "zeros", "inf", "subnormal")


@pytest.fixture(scope="module")
def eng():
    torch.cuda.set_device(0)
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


def _scores(rng, n, kind):
    if kind == "equal":
        return np.full(n, 0.5, np.float32)
    v = (rng.integers(0, 50, n) / 50.0).astype(np.float32)
    if kind == "nan_runs":
        v[rng.random(n) < 0.3] = np.nan
        for s in range(int(rng.integers(0, 40)), n, 997):
            v[s:s + 300] = np.nan
    elif kind == "zeros":
        v = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 0.125, -0.125], np.float32), n)
    elif kind == "inf":
        pick = rng.random(n)
        v[pick < 0.05] = np.inf
        v[(pick >= 0.05) & (pick < 0.2)] = -np.inf
        v[(pick >= 0.2) & (pick < 0.25)] = np.nan
    elif kind == "subnormal":
        b = rng.integers(0, 64, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)    # few distinct: ties
        b[rng.random(n) < 0.1] = 0x00800000                                                             # smallest normal
        v = b.view(np.float32)
    return v


def _expect(ov, yaw, ids, k, thr, offset):
    """(k, 4) int32 records in decide_top_k's order (the oracle of the ranked list)."""
    n = len(ov)
    order = [i for i, _, _ in lcd.decide_top_k(np.arange(n), ov, np.zeros(n), k, None)]
    out = np.tile(np.array([-1, 0, 0, 0], np.int32), (k, 1))
    bits = ov.view(np.int32)
    for r, i in enumerate(order):
        out[r] = [ids[i] if ids is not None else i + offset, bits[i], yaw[i] if yaw is not None else 0, int(ov[i] > np.float32(thr))]
    return out


def _sizes(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 1023, 1024, 1025, 100003, (1 << 20) + 7})


@pytest.mark.parametrize("k", KS)
def test_top_k_matches_the_host_order(eng, k):
    rng = np.random.default_rng(k)
    dev = eng.device
    case = 0
    for n in _sizes(k):
        for kind in KINDS:
            if n > 200000 and kind not in ("ties", "nan_runs", "equal"):
                continue
            case += 1
            ov = _scores(rng, n, kind)
            yaw = rng.integers(-179, 181, n).astype(np.int32)
            ids = rng.integers(0, 1 << 30, n).astype(np.int32)
            use_yaw, use_ids, offset = case % 2 == 0, case % 3 == 0, (0 if case % 4 else 1000)
            thr = (0.3, 0.0, float("-inf"), 0.5)[case % 4]
            got = eng.top_k(torch.from_numpy(ov).to(dev), torch.from_numpy(yaw).to(dev) if use_yaw else None, k, thr,
                            ids=torch.from_numpy(ids).to(dev) if use_ids else None, index_offset=offset)
            want = _expect(ov, yaw if use_yaw else None, ids if use_ids else None, k, thr, offset)
            g = got.cpu().numpy()
            assert got.shape == (k, 4) and got.dtype == torch.int32
            for field, name in enumerate(("id", "overlap bits", "yaw", "above")):
                bad = np.nonzero(g[:, field] != want[:, field])[0]
                assert bad.size == 0, "n=%d k=%d %s: %s differs first at record %d: %s vs %s" % (
                    n, k, kind, name, bad[0], g[bad[0]].tolist(), want[bad[0]].tolist())


def test_k1_is_best_match_and_calls_repeat(eng):
    rng = np.random.default_rng(11)
    dev = eng.device
    for n in (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 100003, (1 << 20) + 7):
        for kind in KINDS:
            ov = torch.from_numpy(_scores(rng, n, kind)).to(dev)
            yaw = torch.from_numpy(rng.integers(-179, 181, n).astype(np.int32)).to(dev)
            for thr in (0.3, 0.0):
                a = eng.top_k(ov, yaw, 1, thr, index_offset=7)
                b = eng.best_match(ov, yaw, thr, index_offset=7)
                assert torch.equal(a.reshape(4), b), (n, kind, a.tolist(), b.tolist())
            x = eng.top_k(ov, yaw, 64, 0.3)
            y = eng.top_k(ov, yaw, 64, 0.3)
            assert torch.equal(x, y), (n, kind)


def test_top_k_refusals_and_out(eng):
    dev = eng.device
    ov = torch.rand(100, device=dev)
    with pytest.raises(OvnError, match="k must be"):
        eng.top_k(ov, k=0)
    with pytest.raises(OvnError, match="k must be"):
        eng.top_k(ov, k=1025)
    buf = torch.full((4 * 8 + 1,), 5, dtype=torch.int32, device=dev)
    with pytest.raises(OvnError, match="16-byte aligned"):
        eng.top_k(ov, k=8, out=buf[1:])                           # 4-byte offset
    assert torch.all(buf == 5)                                   # refused before any launch
    with pytest.raises(OvnError, match="out must be"):
        eng.top_k(ov, k=8, out=buf[:16])
    with pytest.raises(OvnError, match="overlap must be"):
        eng.top_k(ov.double(), k=8)
    out = torch.empty((8, 4), dtype=torch.int32, device=dev)
    assert eng.top_k(ov, k=8, out=out) is out
    torch.cuda.synchronize()
    d = decode_top_k(out)
    assert [r[0] for r in d] == torch.argsort(ov, descending=True, stable=True)[:8].tolist()


# ---- through Infer, on the real heads --------------------------------------------------------------------------------------------
def _write_sequence(root, fx, n, rows=1):
    """n frames: frame i = fixture scan (i mod 2) rolled by 40 (i // 2) columns (every `rows`-th beam)."""
    seq = os.path.join(root, "07")
    for sub in ("depth", "normal"):
        os.makedirs(os.path.join(seq, sub), exist_ok=True)
    for i in range(n):
        s, shift = i % 2, 40 * (i // 2)
        np.save(os.path.join(seq, "depth", "%06d.npy" % i), np.ascontiguousarray(np.roll(fx["range_%d" % s], shift, axis=1)[::rows]))
        np.save(os.path.join(seq, "normal", "%06d.npy" % i), np.ascontiguousarray(np.roll(fx["normal_%d" % s], shift, axis=1)[::rows]))


def _config(root, model=None, **extra):
    cfg = {"model": model or dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(root),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    cfg.update(extra)
    return cfg


def _replay(a, b, n, calls):
    """Feeds frames 0 .. n-1 to both objects: `a` through infer_top_k, `b` through infer_multiple (+ decide_top_k) or, where asked,
    infer_best_match.  Returns the number of non-empty top-k lists compared."""
    nonempty = 0
    for i in range(n):
        refs, k, thr, via_best = calls(i)
        if via_best:                                  # the k = 1 invariant: [infer_best_match(...)], or [] where that is None
            got = a.infer_top_k(i, refs, 1, thr)
            m = b.infer_best_match(i, refs, thr)
            assert got == ([m] if m else []), (i, got, m)
            continue
        got = a.infer_top_k(i, refs, k, thr)
        res = b.infer_multiple(i, refs)
        want = [] if res is None else lcd.decide_top_k(refs, res[0], res[1], k, thr)
        assert got == want, (i, refs, k, thr, got, want)
        nonempty += int(len(got) > 0)
    return nonempty


def test_infer_top_k_equals_decide_top_k_on_infer_multiple(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    n = 14
    _write_sequence(str(tmp_path / "data"), fixture_npz, n + 1)
    w = S.make_test_weights(4, seed=0)
    a, b = Infer(_config(tmp_path / "data"), weights=w), Infer(_config(tmp_path / "data"), weights=w)
    # a threshold inside the range the test weights produce: filtering keeps some candidates and drops others
    probe = Infer(_config(tmp_path / "data"), weights=w)
    for i in range(4):
        res = probe.infer_multiple(i, list(range(i)))
    mid = float(np.median(res[0]))
    probe.close()

    def calls(i):
        refs = list(range(i))
        if i == 9:
            refs = [3, 1, 3, 0, 1]                    # duplicate references: equal overlaps, list order decides
        if i == 11:
            refs = []
        k = (1, 5, 64, 3)[i % 4]
        thr = (None, 0.3, mid, -1.0)[i % 4]
        return refs, k, thr, i in (6, 10, 13) and thr is not None
    try:
        assert _replay(a, b, n, calls) >= 7
        assert a.infer_top_k(n, list(range(n)), 1024, None) == lcd.decide_top_k(list(range(n)), *b.infer_multiple(n, list(range(n))), 1024, None)
        with pytest.raises(ValueError):
            a.infer_top_k(n + 1, [0], 0)
    finally:
        a.close()
        b.close()


def test_infer_top_k_at_width_371(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    n = 6
    _write_sequence(str(tmp_path / "data"), fixture_npz, n, rows=2)
    model = dict(S.REFERENCE_MODEL_CFG, inputShape=[32, 900], leg_output_width=371, additional_unsymmetric_layer3a=False)
    w = S.make_test_weights(4, seed=0, model_cfg=model, feat_w=371)
    a = Infer(_config(tmp_path / "data", model=dict(model)), weights=w)
    b = Infer(_config(tmp_path / "data", model=dict(model)), weights=w)
    try:
        assert a.feat_w == 371
        assert _replay(a, b, n, lambda i: (list(range(i)), 3, 0.0 if i % 2 == 0 or i == 5 else None, i == 5)) >= 2
    finally:
        a.close()
        b.close()
