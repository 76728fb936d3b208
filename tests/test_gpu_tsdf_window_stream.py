"""GPU (MI355X): the stream contract of include/ovn_hip.h for the four `ovn_tsdf_window_*` calls, on a NON-default stream.

Their prototypes carry `stream` as the second parameter, as `ovn_tsdf_raycast` does, so the table of tests/test_gpu_stream_contract.py
does not list them; this file makes the table's four checks with the same harness (tests/_stream_harness.py), the way
tests/test_gpu_raycast_stream.py does.  One case, one window: a shift, a fusion into the shifted window, the brick mask of its storage, a
masked cast with every output, and the triangles of the whole window with the count left on the device (`OvnEngine.tsdf_triangles`
reads the count back, which `ovn_tsdf_window_triangles` itself does not)."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _stream_harness as H

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

Case = collections.namedtuple("Case", "call inputs decoys")
CAPACITY = 1 << 15


@pytest.fixture(scope="module")
def world():
    from overlapnet_amd import _lib
    from overlapnet_amd.engine import OvnEngine, _ptr
    from tests import _render_ref as R
    from tests import _tsdf_ref as T
    from tests import _tsdf_window_ref as WR
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    H.calibrate(dev)
    e = OvnEngine(64, 900, 1, device=0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = T.fused_case(WR.CASE)
    old, new = WR.BASE, (WR.BASE[0] + 8, WR.BASE[1], WR.BASE[2] - 8)
    anchor = WR.anchor_for(old)
    nx, ny, nz = WR.SHAPE
    t0, w0 = T.fresh(WR.SHAPE)
    t, w, rng, ps = up(t0), up(w0), up(c["ranges"]), up(c["poses"])
    sensor = (R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE)
    e.tsdf_integrate(t, w, anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, rng[:3], ps[:3], *sensor, base=old)      # the window before the move
    decoys = [torch.full_like(t, 0.25), torch.full_like(w, 2.0), up(c["ranges"][::-1, :, ::-1]), up(c["poses"][::-1])]
    h, wd = c["ranges"].shape[1:]
    org, i3 = (C.c_double * 3)(*anchor), lambda v: (C.c_int32 * 3)(*v)
    top = tuple(b + n - 1 for b, n in zip(new, WR.SHAPE))

    def call():
        e.tsdf_window_shift(t, w, old, new)
        e.tsdf_integrate(t, w, anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, rng, ps, *sensor, base=new)
        mask = e.tsdf_bricks(w, 1.0)
        view = e.tsdf_raycast(t, w, anchor, T.VOXEL, ps[:2], h, wd, R.FOV_UP, R.FOV_DOWN, 0.5, R.MAX_RANGE, T.VOXEL, 1.0, mask,
                              want=("range", "vertex", "normal"), stacked_flags=(True, True), base=new)
        tri = torch.zeros((CAPACITY, 3, 3), dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.check(e.lib.ovn_tsdf_window_triangles(e._h, e._stream(), _ptr(t), _ptr(w), nx, ny, nz, org, i3(new), T.VOXEL, 1.0, i3(new),
                                                   i3(top), _ptr(tri), CAPACITY, _ptr(count)), "ovn_tsdf_window_triangles")
        return t, w, mask, view, tri, count

    case = Case(call, [t, w, rng, ps], decoys)
    reals = [b.clone() for b in case.inputs]
    torch.cuda.synchronize()
    H.run_plain(case.call, case.inputs, reals)                                    # warm-up: tables and scratch reach their size
    torch.cuda.synchronize()
    expected, host = H.run_plain(case.call, case.inputs, reals)
    torch.cuda.synchronize()
    expected_decoy, _ = H.run_plain(case.call, case.inputs, case.decoys)
    torch.cuda.synchronize()
    for b, r in zip(case.inputs, reals):
        b.copy_(r)
    torch.cuda.synchronize()
    assert len(expected) > 0 and not H.same_bits(expected, expected_decoy), "the decoys give the real inputs' result"
    n_tri = int(expected[-1].item())                       # the outputs in harness order: t, w, mask, normal, range, stacked, vertex, tri, count
    assert 0 < n_tri <= CAPACITY and bool((expected[4] > 0).any()), "the case must mesh and see a surface (%d triangles)" % n_tri
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
    print("STREAM tsdf_window: delay %.3f s, warm host time %.6f s, host time behind the delay %.6f s, delay pending at return: %s"
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
