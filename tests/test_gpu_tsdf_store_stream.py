"""GPU (MI355X): the stream contract of include/ovn_hip.h for the three calls of include/ovn_hip_tsdf_store.h, on a NON-default stream.

The prototypes carry their `stream` as the second parameter, so the table of tests/test_gpu_stream_contract.py does not list them; this
file makes the table's four checks for them with the same harness (tests/_stream_harness.py), as tests/test_gpu_deskew_stream.py does for
`ovn_deskew`: the calls are ordered on their stream behind a delay with decoys in their inputs, a deliberately misplaced call is seen,
two streams are used in turn, and the caller's device is restored.  One case: the flags of a whole 72 x 24 x 16 window, a page-out of
some of its bricks into a pool, and a page-in of other bricks from a second pool into a copy of the window."""
import collections

import numpy as np
import pytest
import torch

import _tsdf_window_ref as WR
from tests import _stream_harness as H

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

Case = collections.namedtuple("Case", "call inputs decoys")


@pytest.fixture(scope="module")
def world():
    from overlapnet_amd import tsdf_store as S
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    H.calibrate(dev)
    e = OvnEngine(64, 900, 1, device=0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g = np.random.default_rng(21)
    nx, ny, nz = WR.SHAPE
    base = WR.BASE_NEG

    def window():
        """(tsdf, weight): fresh but for a random half of the bricks, which hold random words."""
        t, w = np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32)
        for z in range(nz // 8):
            for y in range(ny // 8):
                for x in range(nx // 8):
                    if g.random() < 0.5:
                        cut = (slice(8 * z, 8 * z + 8), slice(8 * y, 8 * y + 8), slice(8 * x, 8 * x + 8))
                        t[cut], w[cut] = g.uniform(-1, 1, (8, 8, 8)), g.integers(0, 9, (8, 8, 8))
        return t, w

    keys = np.array([(x, y, z) for z in range(nz // 8) for y in range(ny // 8) for x in range(nx // 8)], np.int32) + np.array(base, np.int32) // 8
    out_keys, in_keys = up(keys[::2]), up(keys[1::3])
    out_slots = up(np.arange(out_keys.shape[0], dtype=np.int32)[::-1])
    in_slots = up(np.arange(in_keys.shape[0], dtype=np.int32))
    pool_words = lambda: g.uniform(-1, 1, in_keys.shape[0] * 1024).astype(np.float32)
    (t, w), (dt, dw) = window(), window()
    tsdf, weight, pool_in = up(t), up(w), up(pool_words())
    decoys = [up(dt), up(dw), up(pool_words())]                 # another window, another pool -- all valid inputs
    box = (tuple(b // 8 for b in base), tuple((b + n) // 8 for b, n in zip(base, WR.SHAPE)))

    def call():
        flags = S.window_brick_flags(e, tsdf, weight, base, *box)
        pool_out = torch.zeros(out_keys.shape[0] * 1024, dtype=torch.float32, device=dev)
        S.window_page_out(e, tsdf, weight, base, out_keys, out_slots, pool_out)
        t2, w2 = tsdf.clone(), weight.clone()
        S.window_page_in(e, t2, w2, base, in_keys, in_slots, pool_in)
        return flags, pool_out, t2, w2

    case = Case(call, [tsdf, weight, pool_in], decoys)
    reals = [b.clone() for b in case.inputs]
    torch.cuda.synchronize()
    H.run_plain(case.call, case.inputs, reals)                                    # warm-up: torch's allocator has its blocks
    torch.cuda.synchronize()
    expected, host = H.run_plain(case.call, case.inputs, reals)
    torch.cuda.synchronize()
    expected_decoy, _ = H.run_plain(case.call, case.inputs, case.decoys)
    torch.cuda.synchronize()
    for b, r in zip(case.inputs, reals):
        b.copy_(r)
    torch.cuda.synchronize()
    assert len(expected) > 0 and not H.same_bits(expected, expected_decoy), "the decoys give the real inputs' result"
    yield dict(dev=dev, case=case, reals=reals, expected=expected, expected_decoy=expected_decoy, host=host, proven=[])
    torch.cuda.synchronize()
    e.close()


def _streams(p, count=1):
    found = H.independent_streams(p["case"].call, p["dev"], count, p["proven"])
    p["proven"] = found + [S for S in p["proven"] if all(S.cuda_stream != f.cuda_stream for f in found)]
    return found


def _restore(p):
    for b, v in zip(p["case"].inputs, p["reals"]):
        b.copy_(v)


def test_calls_are_ordered_on_their_stream(world):
    p, case = world, world["case"]
    _restore(p)
    S, = _streams(p)
    with torch.cuda.stream(S):                              # once on S without a delay: torch's allocator gets its blocks for this stream
        H.run_plain(case.call, case.inputs, p["reals"])
    torch.cuda.synchronize()
    delay = H.case_delay(p["host"])
    got, pending, host = H.run_delayed(case.call, case.inputs, case.decoys, p["reals"], delay_s=delay, stream=S)
    print("STREAM tsdf store: delay %.3f s, warm host time %.6f s, host time behind the delay %.6f s, delay pending at return: %s"
          % (delay, p["host"], host, pending))
    assert len(got) == len(p["expected"])
    for i, (a, b) in enumerate(zip(got, p["expected"])):
        same = torch.equal(H.bits(a), H.bits(b))
        decoy = (not same) and torch.equal(H.bits(a), H.bits(p["expected_decoy"][i]))
        assert same, "output %d differs from the default-stream bits%s" % (i, " and equals the DECOY's result" if decoy else "")
    assert pending, "the call made the host wait: the delay (%.3f s) had completed when it returned after %.3f s" % (delay, host)


def test_the_harness_sees_a_misplaced_call(world):
    p, case = world, world["case"]
    _restore(p)
    S, = _streams(p)
    got, pending, host = H.run_delayed(case.call, case.inputs, case.decoys, p["reals"], delay_s=H.case_delay(p["host"]), stream=S,
                                       misplaced=True)
    assert pending, "the side stream's delay was over when the default stream had drained"
    assert H.same_bits(got, p["expected_decoy"]), "a call on the default stream did not read the decoys"
    assert not H.same_bits(got, p["expected"])


def test_two_streams_in_turn(world):
    p, case = world, world["case"]
    _restore(p)
    S1, S2 = _streams(p, 2)
    for S in (S1, S2):
        with torch.cuda.stream(S):
            H.run_plain(case.call, case.inputs, p["reals"])
        torch.cuda.synchronize()                            # one stream at a time: calls of one context share its scratch
    with torch.cuda.stream(S1):
        H.enqueue_delay(H.TARGET_DELAY_S, p["dev"])
        for b, r in zip(case.inputs, p["reals"]):
            b.copy_(r)
        first = [t.clone() for t in H.tensors_of(case.call())]
        for b, d in zip(case.inputs, case.decoys):
            b.copy_(d)
    S2.wait_stream(S1)
    with torch.cuda.stream(S2):
        again = [t.clone() for t in H.tensors_of(case.call())]                 # reads the decoys S1 left
        for b, r in zip(case.inputs, p["reals"]):
            b.copy_(r)
        third = [t.clone() for t in H.tensors_of(case.call())]
    torch.cuda.synchronize()
    assert H.same_bits(first, p["expected"]), "first call, on S1"
    assert H.same_bits(again, p["expected_decoy"]), "second call, on S2 behind S1"
    assert H.same_bits(third, p["expected"]), "third call, on S2"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU to be the caller's current device")
def test_caller_device_is_restored(world):
    p, case = world, world["case"]
    torch.cuda.synchronize()
    try:
        torch.cuda.set_device(1)
        got, _ = H.run_plain(case.call, case.inputs, p["reals"])
        assert torch.cuda.current_device() == 1, "the call left device %d current" % torch.cuda.current_device()
        torch.cuda.synchronize(p["dev"])
        assert H.same_bits(got, p["expected"])
    finally:
        torch.cuda.set_device(0)
