"""GPU (MI355X): `ovn_grad_reduce_adagrad` (csrc/grad_reduce.hip) against its NumPy restatement tests/_grad_reduce_ref.py, BIT FOR
BIT on the uint32 views of params, accum and grad_out.

  count   1, 3, 4, 5, 1027: less than one 16-byte vector, a tail of 1 and of 3 elements, more than one workgroup plus a tail;
  stride  count rounded up to 4, and that + 8;
  world   1, 2, 3, 8 with weights 1.0; 0.5 / 0.5; 3/8, 3/8, 2/8; eighths -- and for every world > 1 a set with zero weights whose
          rows (like every padding column) are NaN and must not be read;
  values  (tests/_grad_reduce_ref.make_case) gradient magnitudes log-uniform in 1e-12 .. 1e3 with random signs, exact zeros on a
          zero accumulator (the parameter must not move), |g| = 1e-20 (g^2 a float32 denormal), |g| = 1e-25 (g^2 underflows),
          accumulators zero and 1e-8 .. 1e4;
  modes   update with and without grad_out, reduce-only (NULL params / accum), the same bits on a second call, buffers that are not
          16-byte aligned (served element by element), and the Python wrapper's argument checks."""
import numpy as np
import pytest
import torch

from overlapnet_amd import _lib
from tests import _grad_reduce_ref as G

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 5, 1027)
LR, EPS = 2e-4, 1e-7


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(32, 247, 4)           # no weights: the kernel needs a context (device, profiling), nothing else
    yield e
    e.close()


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _same(tag, gpu, ref):
    a, b = _bits(gpu), _bits(ref)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (tag, bad[:8], np.asarray(ref)[bad[:8]], gpu.cpu().numpy()[bad[:8]])


@pytest.mark.parametrize("world", sorted(G.WEIGHT_SETS))
@pytest.mark.parametrize("count", COUNTS)
def test_kernel_is_the_numpy_restatement_bit_for_bit(eng, count, world):
    dev = eng.device
    for weights in G.WEIGHT_SETS[world]:
        for stride in ((count + 3) // 4 * 4, (count + 3) // 4 * 4 + 8):
            c = G.make_case(count, stride, world, weights)
            tag = (count, stride, world, tuple(weights))
            rp, ra, rg = G.reduce_adagrad(c["grads"], c["weights"], count, c["params"], c["accum"], LR, EPS)
            assert np.all(np.isfinite(rp)) and np.all(np.isfinite(ra)) and np.all(np.isfinite(rg)), tag
            g = torch.from_numpy(c["grads"]).to(dev)
            for rep in range(2):                                  # the same bits on a second call
                p, a = torch.from_numpy(c["params"]).to(dev), torch.from_numpy(c["accum"]).to(dev)
                out = eng.grad_reduce_adagrad(g, c["weights"], p, a, LR, EPS, want_grad=True)
                _same(tag + ("params", rep), p, rp)
                _same(tag + ("accum", rep), a, ra)
                _same(tag + ("grad_out", rep), out, rg)
            # exact zeros on a zero accumulator do not move the parameter
            z = (rg == 0) & (c["accum"] == 0)
            assert np.array_equal(_bits(p)[z], c["params"].view(np.uint32)[z])
            # no grad_out: the same update
            p, a = torch.from_numpy(c["params"]).to(dev), torch.from_numpy(c["accum"]).to(dev)
            assert eng.grad_reduce_adagrad(g, c["weights"], p, a, LR, EPS) is None
            _same(tag + ("params", "no grad_out"), p, rp)
            _same(tag + ("accum", "no grad_out"), a, ra)
            # reduce only: NULL params / accum
            only = eng.grad_reduce_adagrad(g, c["weights"], count=count)
            assert only.numel() == count
            _same(tag + ("reduce only",), only, rg)


def test_unaligned_buffers_take_the_scalar_form(eng):
    """Views that start 4 bytes into an allocation: no 16-byte access is possible, the bits stay the same."""
    dev = eng.device
    count, stride, world = 1027, 1028, 3
    c = G.make_case(count, stride, world, [3 / 8, 3 / 8, 2 / 8], seed=1)
    rp, ra, rg = G.reduce_adagrad(c["grads"], c["weights"], count, c["params"], c["accum"], LR, EPS)
    g = torch.from_numpy(c["grads"]).to(dev)
    pbuf = torch.zeros(count + 1, dtype=torch.float32, device=dev)
    abuf = torch.zeros(count + 1, dtype=torch.float32, device=dev)
    p, a = pbuf[1:], abuf[1:]
    p.copy_(torch.from_numpy(c["params"]))
    a.copy_(torch.from_numpy(c["accum"]))
    assert p.data_ptr() % 16 == 4
    out = eng.grad_reduce_adagrad(g, c["weights"], p, a, LR, EPS, want_grad=True)
    _same("unaligned params", p, rp)
    _same("unaligned accum", a, ra)
    _same("unaligned grad_out", out, rg)
    assert float(pbuf[0]) == 0.0 and float(abuf[0]) == 0.0


def test_kernel_reports_under_the_profile(eng):
    dev = eng.device
    c = G.make_case(1027, 1028, 2, [0.5, 0.5])
    g = torch.from_numpy(c["grads"]).to(dev)
    eng.profile_begin()
    eng.grad_reduce_adagrad(g, c["weights"], count=1027)
    prof = eng.profile_end()
    assert prof["leg_conv"][1] == 1 and prof["leg_conv"][0] > 0 and sum(v[1] for v in prof.values()) == 1, prof


def test_wrapper_argument_checks(eng):
    dev = eng.device
    g = torch.zeros((2, 8), dtype=torch.float32, device=dev)
    p, a = torch.zeros(6, dtype=torch.float32, device=dev), torch.zeros(6, dtype=torch.float32, device=dev)
    before = p.clone()
    for bad in (lambda: eng.grad_reduce_adagrad(g.cpu(), [0.5, 0.5], p, a),
                lambda: eng.grad_reduce_adagrad(g.double(), [0.5, 0.5], p, a),
                lambda: eng.grad_reduce_adagrad(g[:, ::2], [0.5, 0.5]),
                lambda: eng.grad_reduce_adagrad(g, [1.0], p, a),
                lambda: eng.grad_reduce_adagrad(g, [0.5, 0.5], p, None),
                lambda: eng.grad_reduce_adagrad(g, [0.5, 0.5], p, a[:5]),
                lambda: eng.grad_reduce_adagrad(g, [0.5, 0.5], torch.zeros(9, dtype=torch.float32, device=dev),
                                                torch.zeros(9, dtype=torch.float32, device=dev)),
                lambda: eng.grad_reduce_adagrad(g, [0.5, 0.5], count=9),
                lambda: eng.grad_reduce_adagrad(g, [0.0, 0.0], p, a),
                lambda: eng.grad_reduce_adagrad(g, [1.5, -0.5], p, a),
                lambda: eng.grad_reduce_adagrad(g, [0.5, 0.5], p, a, lr=float("nan")),
                lambda: eng.grad_reduce_adagrad(g, [0.5, 0.5], p, a, eps=-1.0),
                lambda: eng.grad_reduce_adagrad(torch.zeros((2, 6), dtype=torch.float32, device=dev), [0.5, 0.5], p, a)):
        with pytest.raises(_lib.OvnError):
            bad()
    assert torch.equal(p, before)
