"""TEST INFRASTRUCTURE: `ovn_grad_reduce_adagrad` (csrc/grad_reduce.hip) restated in NumPy -- the yardstick the kernel is held to
BIT FOR BIT -- and the inputs the host and GPU tests share.

The sum runs in float64 in rank order (one rounded multiply, one rounded add per rank: NumPy forms no FMA), rows with weight 0.0
are never touched, and the sum is rounded once to float32.  The update is Keras 2.1.5's Adagrad as `train.adagrad_step` states it, on
`np.float32` arrays and scalars, so that each of its five operations (g g, a + ., lr g, sqrt(a) + eps, the divide and the
subtraction) is one correctly rounded float32 operation, denormals included."""
import numpy as np


def reduce_rows(grads, weights, count):
    """grads (world, stride) float32, weights (world) -> (count) float32: the share-weighted sum, fp64 in rank order, rounded once."""
    grads = np.asarray(grads, np.float32)
    s = np.zeros(int(count), np.float64)
    for r, w in enumerate(np.asarray(weights, np.float64)):
        if w == 0.0:
            continue                    # not read: the row may hold anything
        s = s + w * grads[r, :count].astype(np.float64)
    with np.errstate(under="ignore", over="ignore"):
        return s.astype(np.float32)


def reduce_adagrad(grads, weights, count, params=None, accum=None, lr=0.0, eps=1e-7):
    """-> (params, accum, grad_out) as new float32 arrays; params / accum None: (None, None, grad_out)."""
    g = reduce_rows(grads, weights, count)
    if params is None:
        return None, None, g
    p, a = np.asarray(params, np.float32), np.asarray(accum, np.float32)
    lr32, eps32 = np.float32(lr), np.float32(eps)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        gg = g * g
        a = a + gg
        num = lr32 * g
        den = np.sqrt(a) + eps32
        p = p - num / den
    assert p.dtype == np.float32 and a.dtype == np.float32
    return p, a, g


WEIGHT_SETS = {1: [[1.0]], 2: [[0.5, 0.5], [1.0, 0.0]], 3: [[3 / 8, 3 / 8, 2 / 8], [0.5, 0.0, 0.5]],
               8: [[1 / 8] * 8, [3 / 16, 0.0, 3 / 16, 2 / 16, 0.0, 3 / 16, 3 / 16, 2 / 16]]}


def make_case(count, stride, world, weights, seed=0):
    """Inputs of one case -> dict grads (world, stride), weights, params, accum (count).  Gradient magnitudes log-uniform in
    1e-12 .. 1e3 with random signs; every position that is 0 mod 7 is an exact zero in every row with a zero accumulator (the
    parameter must not move), 1 mod 7 holds |g| = 1e-20 (g^2 is a float32 denormal), 2 mod 7 holds |g| = 1e-25 (g^2 underflows);
    accumulators are zero at 3 mod 7 as well and log-uniform in 1e-8 .. 1e4 elsewhere.  Rows with weight 0.0 and the padding
    columns are NaN."""
    rng = np.random.default_rng([seed, count, stride, world])
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    g = (10.0 ** rng.uniform(-12, 3, (world, stride))) * sign((world, stride))
    i = np.arange(stride)
    g[:, i % 7 == 0] = 0.0
    g[:, i % 7 == 1] = 1e-20 * sign((world, int(np.sum(i % 7 == 1))))
    g[:, i % 7 == 2] = 1e-25 * sign((world, int(np.sum(i % 7 == 2))))
    g = g.astype(np.float32)
    g[:, count:] = np.nan
    w = np.asarray(weights, np.float64)
    g[w == 0.0] = np.nan
    a = (10.0 ** rng.uniform(-8, 4, count)).astype(np.float32)
    j = np.arange(count)
    a[(j % 7 == 0) | (j % 7 == 3)] = 0.0
    a[(j % 7 == 1) & (j % 2 == 0)] = 0.0
    p = rng.normal(0.0, 0.1, count).astype(np.float32)
    return {"grads": g, "weights": w, "params": p, "accum": a}
