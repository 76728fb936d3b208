"""CPU: the host side of data-parallel training.

  - the header declares `ovn_grad_reduce_adagrad`, the library exports it, the binding lists it, the ABI version is still 11;
  - every argument error the header lists is refused before any HIP call (NULL context or buffers: no GPU is needed);
  - the yardstick tests/_grad_reduce_ref.py: at world 1 with weight 1.0 it is `train.adagrad_step` on CPU float32 tensors bit for
    bit (CPU torch rounds every operation correctly), and a zero-weight row full of NaN leaves the result untouched;
  - `distributed.exchange_gradients` at world 3 under gloo with shares 3/3/2, with 1/1/0 and with one rank reporting a status: rows
    in rank order, weights n_r / n, the loss the weighted sum, the same statuses on every rank;
  - the pair split covers a batch exactly once for n = 0..20, world = 1..5;
  - `DataParallelTrainer` exists, derives from `OverlapNetTrainer` and refuses a sharded `Infer`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from overlapnet_amd import _lib
from overlapnet_amd import distributed as D
from tests import _grad_reduce_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    assert re.search(r"int ovn_grad_reduce_adagrad\(ovn_ctx\* ctx, const float\* grads_dev, int world, int64_t stride, "
                     r"const double\* rank_weight_host,\s+int64_t count, float\* params_dev, float\* accum_dev, float lr, float eps, "
                     r"float\* grad_out_dev, void\* stream\);", src)
    assert int(re.search(r"#define OVN_ABI_VERSION (\d+)", src).group(1)) == 11 == _lib.ABI_VERSION
    assert int(re.search(r"#define OVN_GRAD_REDUCE_MAX_WORLD (\d+)", src).group(1)) == 64
    res, args = _lib.SIGNATURES["ovn_grad_reduce_adagrad"]
    assert res is C.c_int and len(args) == 12 and args[4] == C.POINTER(C.c_double)
    lib = _lib.load()
    assert lib.ovn_abi_version() == 11
    assert hasattr(lib, "ovn_grad_reduce_adagrad")
    from overlapnet_amd.engine import OvnEngine
    assert OvnEngine.GRAD_REDUCE_MAX_WORLD == 64 and callable(OvnEngine.grad_reduce_adagrad)


# a pointer value that is never dereferenced: every case below is refused before the context or a buffer is touched
FAKE = C.c_void_p(4096)


def _call(ctx=None, grads=FAKE, world=2, stride=8, weights=(0.5, 0.5), count=6, params=FAKE, accum=FAKE, lr=0.1, eps=1e-7, out=FAKE):
    lib = _lib.load()
    w = None if weights is None else (C.c_double * len(weights))(*weights)
    rc = lib.ovn_grad_reduce_adagrad(ctx, grads, world, stride, w, count, params, accum, lr, eps, out, None)
    return rc, lib.ovn_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(), "NULL argument"),                                        # the context
    (dict(grads=None), "NULL argument"),
    (dict(weights=None), "NULL argument"),
    (dict(world=0), "world"), (dict(world=65, weights=(1 / 65,) * 65), "world"),
    (dict(count=0), "count"),
    (dict(stride=4, count=6), "stride"), (dict(stride=7, count=6), "stride"),
    (dict(params=None), "together"), (dict(accum=None), "together"),
    (dict(params=None, accum=None, out=None), "no output"),
    (dict(lr=float("nan")), "finite"), (dict(lr=float("inf")), "finite"), (dict(eps=float("inf")), "finite"), (dict(eps=-1e-7), "finite"),
    (dict(weights=(1.5, -0.5)), "negative or not finite"), (dict(weights=(float("nan"), 1.0)), "negative or not finite"),
    (dict(weights=(float("inf"), 0.0)), "negative or not finite"),
    (dict(weights=(0.0, 0.0)), "zero"),
], ids=lambda v: "-".join("%s" % k for k in v) if isinstance(v, dict) else None)
def test_argument_errors_before_any_hip_call(kw, msg):
    rc, err = _call(**kw)
    assert rc == 1 and msg in err, (rc, err)


def test_reference_is_adagrad_step_at_world_one():
    from overlapnet_amd.train import adagrad_step
    for count in (1, 5, 1027):
        c = G.make_case(count, count + 3 & ~3, 1, [1.0], seed=3)
        p, a, g = G.reduce_adagrad(c["grads"], c["weights"], count, c["params"], c["accum"], lr=2e-4, eps=1e-7)
        assert np.array_equal(g.view(np.uint32), c["grads"][0, :count].view(np.uint32))       # 1.0 * g in fp64 and back: exact
        tp, ta = torch.from_numpy(c["params"].copy()), torch.from_numpy(c["accum"].copy())
        adagrad_step([tp], [ta], [torch.from_numpy(c["grads"][0, :count].copy())], 2e-4)
        assert np.array_equal(a.view(np.uint32), ta.numpy().view(np.uint32))
        assert np.array_equal(p.view(np.uint32), tp.numpy().view(np.uint32))
        # the fixture holds what the GPU test relies on: zeros that must not move, denormal and underflowing squares
        z = (g == 0) & (c["accum"] == 0)
        assert z.any() and np.array_equal(p[z], c["params"][z])
        if count > 7:
            sq = g.astype(np.float32) * g.astype(np.float32)
            assert ((sq > 0) & (sq < np.finfo(np.float32).tiny)).any() and ((sq == 0) & (g != 0)).any()


def test_reference_never_reads_a_zero_weight_row():
    c = G.make_case(1027, 1036, 3, [0.5, 0.0, 0.5], seed=4)
    assert np.all(np.isnan(c["grads"][1])) and np.all(np.isnan(c["grads"][:, 1027:]))
    p, a, g = G.reduce_adagrad(c["grads"], c["weights"], 1027, c["params"], c["accum"], lr=1e-3)
    two = np.stack([c["grads"][0], c["grads"][2]])
    p2, a2, g2 = G.reduce_adagrad(two, [0.5, 0.5], 1027, c["params"], c["accum"], lr=1e-3)
    for x, y in ((p, p2), (a, a2), (g, g2)):
        assert np.all(np.isfinite(x)) and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # the sum is weighted and ordered: 3/8, 3/8, 2/8 of three rows in fp64, rounded once
    c = G.make_case(5, 8, 3, [3 / 8, 3 / 8, 2 / 8], seed=5)
    want = ((0.375 * c["grads"][0, :5].astype(np.float64) + 0.375 * c["grads"][1, :5].astype(np.float64))
            + 0.25 * c["grads"][2, :5].astype(np.float64)).astype(np.float32)
    assert np.array_equal(G.reduce_rows(c["grads"], c["weights"], 5).view(np.uint32), want.view(np.uint32))
    _, _, only = G.reduce_adagrad(c["grads"], c["weights"], 5)
    assert np.array_equal(only.view(np.uint32), want.view(np.uint32))


def test_pair_split_covers_a_batch_exactly_once():
    for world in range(1, 6):
        for n in range(0, 21):
            seen = []
            for r in range(world):
                lo, hi = D.shard_bounds(n, world, r)
                assert 0 <= lo <= hi <= n
                seen += list(range(lo, hi))
            assert seen == list(range(n)), (n, world)
            sizes = D.shard_sizes(n, world)
            assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)      # idle ranks, if any, are the last


def test_payload_layout():
    for count in (1, 3, 4, 5, 1027):
        row = D.grad_row_floats(count)
        assert row % 4 == 0 and row - D.GRAD_TRAILER >= count and row - D.GRAD_TRAILER - count < 4
    # without a process group the call is world 1 and moves nothing
    flat = torch.arange(5, dtype=torch.float32)
    rows, w, loss, st = D.exchange_gradients(flat, 7, (0.25, 0.5), 0)
    assert rows.shape == (1, 12) and torch.equal(rows[0, :5], flat) and list(w) == [1.0] and loss == 0.75 and list(st) == [0]
    lss, counts, st = D.unpack_grad_trailer(rows)
    assert lss.tolist() == [[0.25, 0.5]] and counts.tolist() == [7] and st.tolist() == [0]


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


COUNT = 1027


def _rank_flat(rank):
    return torch.from_numpy(np.random.default_rng([11, rank]).normal(0, 1, COUNT).astype(np.float32))


def _rank_losses(rank):
    return (0.5 + 0.125 * rank, 0.03125 * (rank + 1))


def _worker_exchange(rank, world, port, shares, bad_rank, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        status = 7 if rank == bad_rank else 0
        flat = _rank_flat(rank) if shares[rank] else torch.full((COUNT,), float("nan"))
        rows, w, loss, statuses = D.exchange_gradients(flat, shares[rank], _rank_losses(rank), status)
        q.put((rank, rows.numpy().copy(), np.asarray(w), float(loss), np.asarray(statuses)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("shares,bad_rank", [((3, 3, 2), None), ((1, 1, 0), None), ((3, 3, 2), 1)], ids=["3-3-2", "1-1-0", "rank1-fails"])
def test_exchange_gradients_world3_gloo(shares, bad_rank):
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_exchange, args=(r, world, port, shares, bad_rank, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    good = [0 if r == bad_rank else shares[r] for r in range(world)]
    n = sum(good)
    want_w = np.array([s / n for s in good], np.float64)
    want_loss = 0.0
    for r in range(world):
        if good[r]:
            lo = _rank_losses(r)
            want_loss = want_loss + want_w[r] * (np.float64(np.float32(lo[0])) + np.float64(np.float32(lo[1])))
    for rank, rows, w, loss, statuses in got:
        assert rows.shape == (world, D.grad_row_floats(COUNT)) and rows.dtype == np.float32
        for r in range(world):
            if shares[r]:
                assert np.array_equal(rows[r, :COUNT].view(np.uint32), _rank_flat(r).numpy().view(np.uint32)), (rank, r)    # rank order
        assert np.array_equal(w, want_w), (rank, w)
        assert loss == want_loss, (rank, loss, want_loss)
        assert statuses.tolist() == [7 if r == bad_rank else 0 for r in range(world)]
        # every rank holds the same payload, bit for bit
        assert np.array_equal(rows.view(np.uint32), got[0][1].view(np.uint32))
        # the reference on these rows never reads the idle rank's NaN row
        if bad_rank is None:
            g = G.reduce_rows(rows, w, COUNT)
            assert np.all(np.isfinite(g))


def test_trainer_class_and_its_refusals(monkeypatch):
    from overlapnet_amd.train import DataParallelTrainer, OverlapNetTrainer
    assert issubclass(DataParallelTrainer, OverlapNetTrainer)

    class Sharded(object):
        _world = 2
    with pytest.raises(_lib.OvnError):
        DataParallelTrainer(Sharded(), 1e-3)

    class Plain(object):
        _world = 1
    monkeypatch.setenv("WORLD_SIZE", "2")                 # a launcher's environment, but no init_process_group
    with pytest.raises(_lib.OvnError, match="not initialised"):
        DataParallelTrainer(Plain(), 1e-3)
