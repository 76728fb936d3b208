"""CPU: the host side of batched loop-closure queries -- the segment-table checks of `OvnEngine.heads_segments` / `top_k_segments`,
the refusals of the `Infer.*_batch` methods before any GPU work (ids out of range, k outside 1..1024, a sharded object), the C ABI's
refusals (no GPU call), and `lcd.detect_offline` against the `lcd.detect` loop on a host fake of `Infer`."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from overlapnet_amd import _lib
from overlapnet_amd import lcd
from overlapnet_amd.engine import check_top_k, segment_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segment_table_accepts_csr_batches():
    o, q = segment_table([0, 0, 3, 3, 10], [4, 0, 1, 2], 5)
    assert o.dtype == np.int64 and o.tolist() == [0, 0, 3, 3, 10] and o.flags.c_contiguous
    assert q.dtype == np.int32 and q.tolist() == [4, 0, 1, 2]
    o, q = segment_table(np.array([0], np.int32), [], 0)           # B = 0
    assert o.tolist() == [0] and q.size == 0
    o, _ = segment_table([0, 2, 2], None, None)                     # top_k_segments: offsets only
    assert o.tolist() == [0, 2, 2]


@pytest.mark.parametrize("offs", [[1, 2], [0, 3, 2], [0, 5, 4, 6], [], [0.0, 1.5]])
def test_segment_table_refuses_bad_offsets(offs):
    with pytest.raises(ValueError):
        segment_table(offs, None, None)


def test_segment_table_refuses_bad_queries():
    with pytest.raises(IndexError):
        segment_table([0, 1, 2], [0, 5], 5)                         # index out of range
    with pytest.raises(IndexError):
        segment_table([0, 1, 2], [-1, 0], 5)
    with pytest.raises(ValueError):
        segment_table([0, 1, 2], [0], 5)                            # one query per segment


@pytest.mark.parametrize("k", [0, -1, 1025, 4096])
def test_k_outside_1_to_1024_is_refused(k):
    with pytest.raises(ValueError):
        check_top_k(k)
    assert check_top_k(1) == 1 and check_top_k(1024) == 1024


def test_c_abi_segment_refusals_without_gpu_calls():
    h = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    assert "#define OVN_ABI_VERSION 11" in h and _lib.ABI_VERSION == 11
    assert int(re.search(r"#define OVN_SEG_PASS_MAX (\d+)", h).group(1)) >= 1
    lib = _lib.load()
    offs = (C.c_int64 * 3)(0, 2, 1)
    assert lib.ovn_top_k_segments(None, None, None, None, offs, 2, 1, 0.3, None, None) == 1
    assert b"ctx is NULL" in lib.ovn_last_error()
    assert lib.ovn_heads_segments(None, *([None] * 7), offs, 2, 1, None, None, None, None, None) == 3   # no context: state error


class _FakeInfer:
    """Host stand-in for `Infer`: overlap of (candidate, query) a fixed function of the two frame ids, yaw their difference --
    with infer_best_match (what `lcd.detect` calls) and cache_frames / infer_best_match_batch (what `lcd.detect_offline` calls)
    holding the same rule: NumPy's first maximum, `> overlap_thres`."""

    def __init__(self):
        self.cached = 0
        self.batches = 0

    @staticmethod
    def _score(c, q):
        return np.float32(((c * 7919 + q * 104729) % 1000) / 1000.0)

    def _best(self, cur, refs, thr):
        if len(refs) == 0:
            return None
        ov = np.array([self._score(c, cur) for c in refs], np.float32)
        k = int(np.argmax(ov))
        return (int(refs[k]), float(ov[k]), int(cur - refs[k])) if ov[k] > np.float32(thr) else None

    def infer_best_match(self, cur, refs, thr=0.3):
        assert cur == self.cached and all(0 <= r < cur for r in refs)
        self.cached += 1
        return self._best(cur, refs, thr)

    def cache_frames(self, n):
        self.cached = max(self.cached, n)

    def infer_best_match_batch(self, cur_ids, lists, thr=0.3):
        self.batches += 1
        assert all(0 <= c < self.cached for c in cur_ids) and all(0 <= r < self.cached for l in lists for r in l)
        return [self._best(c, l, thr) for c, l in zip(cur_ids, lists)]


def test_detect_offline_equals_the_detect_loop_on_a_host_fake():
    rng = np.random.default_rng(2)
    n = 400
    xy = np.cumsum(rng.normal(0, 1.0, size=(n, 2)), axis=0)
    xy[300:] = xy[:100] + rng.normal(0, 0.3, size=(100, 2))
    length = lcd.travelled_distances(xy)
    ell = lcd.covariance_ellipse(np.eye(2) * 9.0)
    for kw in ({}, {"overlap_thres": 0.6, "inactive_dist_thres": 10.0}, {"inactive_time_thres": 50}):
        a, b = _FakeInfer(), _FakeInfer()
        loop = [lcd.detect(a, i, xy, length, ell, **dict(kw)) for i in range(n)]
        got = lcd.detect_offline(b, range(n), xy, length, ell, **dict(kw))
        assert got == loop and b.batches == 1 and b.cached == n
        assert any(x is not None for x in loop)
    assert lcd.detect_offline(_FakeInfer(), [], xy, length, ell) == []


def _bare_infer(world=1, n_cached=10):
    """An `Infer` without its GPU half: enough state for the batch methods' host checks."""
    from overlapnet_amd.infer import Infer

    class _Cache:
        def __len__(self):
            return n_cached
    inf = Infer.__new__(Infer)
    inf._world, inf._rank = world, 0
    inf._feature_volumes = _Cache()
    return inf


def test_infer_batch_refusals_before_any_gpu_work():
    inf = _bare_infer()
    for call in (lambda: inf.infer_multiple_batch([3, 10], [[0], [1]]),        # query not cached
                 lambda: inf.infer_best_match_batch([3], [[0, 10]]),           # reference not cached
                 lambda: inf.infer_top_k_batch([3], [[-1]], 5)):               # negative id
        with pytest.raises(IndexError):
            call()
    with pytest.raises(ValueError):
        inf.infer_top_k_batch([3], [[0]], 0)
    with pytest.raises(ValueError):
        inf.infer_top_k_batch([3], [[0]], 1025)
    with pytest.raises(ValueError):
        inf.infer_multiple_batch([3, 4], [[0]])                                # one list per query
    # empty lists need no GPU: the single-query answers for an empty list
    assert inf.infer_multiple_batch([1, 2], [[], []]) == [None, None]
    assert inf.infer_best_match_batch([1], [[]]) == [None]
    assert inf.infer_top_k_batch([1, 2], [[], []], 3) == [[], []]
    sharded = _bare_infer(world=2)
    for call in (lambda: sharded.infer_multiple_batch([1], [[0]]), lambda: sharded.infer_best_match_batch([1], [[0]]),
                 lambda: sharded.infer_top_k_batch([1], [[0]], 2), lambda: sharded.cache_frames(5)):
        with pytest.raises(Exception, match="shard"):
            call()
