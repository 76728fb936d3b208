"""Helper of tests/test_gpu_stream_contract.py: one engine call made on a side stream behind a delay, with decoy inputs.

The header's stream contract (include/ovn_hip.h, "Conventions") says that a call only ENQUEUES work on the stream it is given.  On the
legacy default stream none of that can be observed, so the call is made under `with torch.cuda.stream(S)` and three things are arranged
around it:

  nothing runs ahead of the stream   every input buffer holds a DECOY (valid data of the same shape and dtype that differs from the
                                     real input) until S itself, behind a delay, copies the real input in.  Whatever part of the
                                     call lands on another stream reads decoys.
  nothing lags behind the stream     straight after the call S clones the outputs and writes the decoys back.  A side stream that
                                     was not joined reads decoys or misses the clone.  A race by nature: a best-effort detector.
  the host did not wait              an event E is recorded on S right behind the delay; when the Python call returns, E must
                                     still be pending.

The delay is `torch.cuda._sleep`, calibrated once per process with two events; a build on which `_sleep` does not delay gets a chain of
element-wise torch kernels on a private tensor instead, timed the same way.  No graph capture, no profiler."""
import gc
import math
import time

import torch

TARGET_DELAY_S = 0.1          # the delay every case starts from
HOST_FACTOR = 4.0             # a case whose warm host time is more than a quarter of that gets HOST_FACTOR times its host time
_PROBE_CYCLES = 20_000_000
_CHAIN_ELEMS = 1 << 26        # the fallback's private tensor: 256 MB, one pass over it is some 0.1 ms of HBM time

_delay = {}                   # device index -> ("sleep", seconds per cycle) | ("chain", seconds per op, tensor)


def tensors_of(result):
    """The device tensors of a call's result (a tensor, or a list / tuple / dict of results; None entries dropped), in a fixed order."""
    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, dict):
        return [t for k in sorted(result) for t in tensors_of(result[k])]
    if isinstance(result, (list, tuple)):
        return [t for r in result for t in tensors_of(r)]
    raise TypeError("a call must return device tensors, not %r" % type(result))


def bits(t):
    """The tensor's bit pattern as integers: NaN payloads and the sign of zero count."""
    t = t.contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16)
    return t


def same_bits(a, b):
    """Two lists of tensors, equal bit for bit."""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def _timed(fn, device):
    """Seconds of GPU time `fn` enqueues on the current stream, by two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(device)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def calibrate(device):
    """Finds out, once per device, how this build delays a stream; -> ("sleep" | "chain", seconds per unit)."""
    key = torch.device(device).index or 0
    if key in _delay:
        return _delay[key][:2]
    with torch.cuda.device(key):
        mode = None
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)                                            # the first launch pays for loading the kernel
            t = _timed(lambda: torch.cuda._sleep(_PROBE_CYCLES), key)
            if t >= 1e-3:                                                      # 2e7 cycles of any plausible clock are milliseconds
                mode = ("sleep", t / _PROBE_CYCLES)
        if mode is None:
            x = torch.ones(_CHAIN_ELEMS, dtype=torch.float32, device="cuda:%d" % key)
            x.mul_(1.0)
            t = _timed(lambda: [x.mul_(1.0) for _ in range(20)], key)
            mode = ("chain", t / 20, x)
    _delay[key] = mode
    print("stream harness: delay by %s, %.3g s per %s" % (mode[0], mode[1], "cycle" if mode[0] == "sleep" else "pass"))
    return mode[:2]


def enqueue_delay(seconds, device):
    """Keeps the current stream of `device` busy for about `seconds`."""
    calibrate(device)
    mode = _delay[torch.device(device).index or 0]
    units = max(1, int(math.ceil(seconds / mode[1])))
    if mode[0] == "sleep":
        torch.cuda._sleep(units)
    else:
        for _ in range(units):
            mode[2].mul_(1.0)


def measured_delay(seconds, device):
    """What `enqueue_delay(seconds)` really takes on this device, in seconds (printed by the test module once)."""
    return _timed(lambda: enqueue_delay(seconds, device), device)


def case_delay(host_seconds):
    """The delay of a case whose warm call keeps the host busy for `host_seconds`."""
    return max(TARGET_DELAY_S, HOST_FACTOR * host_seconds)


PROBE_DELAY_S = 0.05          # the delay of an independence probe: well above the GPU time of a call of the table (milliseconds)
MAX_CANDIDATES = 32           # torch hands out its pool of 32 streams per device in turn


def is_independent(S, op, device, delay_s=PROBE_DELAY_S):
    """Does work that `op()` enqueues from the DEFAULT stream run without waiting for work on S?

    The runtime multiplexes its streams over a few hardware queues, and a queue runs in submission order.  Where S shares a queue with
    the default stream -- or with a stream that `op` itself forks onto and joins -- work submitted there lands BEHIND whatever S holds,
    and a launch that ignored its stream argument would be ordered as if it had not: on such an S the decoy scheme proves nothing.  The
    probe: a delay on S, `op()` on the default stream, the default stream ALONE synchronised; S is independent iff the delay's event is
    still pending then."""
    torch.cuda.synchronize(device)
    E = torch.cuda.Event()
    with torch.cuda.stream(S):
        enqueue_delay(delay_s, device)
        E.record(S)
    op()
    torch.cuda.default_stream(device).synchronize()
    pending = not E.query()
    torch.cuda.synchronize(device)
    return pending


def independent_streams(op, device, count=1, proven=()):
    """`count` distinct streams that `is_independent` holds for `op`, those of `proven` tried first; asserts that it found them."""
    found, seen = [], set()
    fresh = (torch.cuda.Stream(device=device) for _ in range(MAX_CANDIDATES))
    for S in list(proven) + [None] * MAX_CANDIDATES:
        if S is None:
            S = next(fresh)
        if S.cuda_stream in seen or S.cuda_stream == torch.cuda.default_stream(device).cuda_stream:
            continue
        seen.add(S.cuda_stream)
        if is_independent(S, op, device):
            found.append(S)
            if len(found) == count:
                return found
    assert False, ("%d of %d streams tried run independently of the default stream and of the streams the call uses, %d needed"
                   % (len(found), len(seen), count))


def run_plain(call, inputs, values):
    """The call on the current stream with `values` in the input buffers -> (clones of its outputs, host seconds of the call)."""
    for buf, v in zip(inputs, values):
        buf.copy_(v)
    t0 = time.perf_counter()
    out = call()
    host = time.perf_counter() - t0
    return [t.clone() for t in tensors_of(out)], host


def run_delayed(call, inputs, decoys, reals=None, delay_s=TARGET_DELAY_S, stream=None, misplaced=False):
    """Makes `call()` under `with torch.cuda.stream(S)` behind a delay, as the module docstring describes.

    inputs   the device buffers the call reads; they hold the real values again on return
    reals    the real values, one device tensor per buffer (default: what the buffers hold on entry -- a call that updates one of its
             inputs in place leaves its RESULT there, so a caller that has run it before passes the values it kept)
    decoys   one device tensor per buffer, same shape and dtype: what the buffers hold whenever S is not inside the call
    stream   S (a fresh torch.cuda.Stream by default)
    misplaced=True makes the call OUTSIDE the `with` block, on the default stream, and waits for the default stream alone before it
    looks at E: the form of a call that ignores its stream argument (tests the harness itself).

    -> (clones of the outputs, was E still pending when the call returned, host seconds of the call)"""
    assert len(inputs) == len(decoys)
    dev = inputs[0].device
    S = stream if stream is not None else torch.cuda.Stream(device=dev)
    reals = [(b if reals is None else reals[i]).clone() for i, b in enumerate(inputs)]     # device-resident: copying them in needs no host
    for buf, d in zip(inputs, decoys):
        assert buf.shape == d.shape and buf.dtype == d.dtype and buf.device == d.device
        buf.copy_(d)
    torch.cuda.synchronize(dev)
    E = torch.cuda.Event()
    gc_was_on = gc.isenabled()
    gc.collect()                 # a collection of the interpreter's inside the timed call would read as a host wait
    gc.disable()
    try:
        with torch.cuda.stream(S):
            enqueue_delay(delay_s, dev)
            E.record(S)
            for buf, r in zip(inputs, reals):
                buf.copy_(r)
            if not misplaced:
                t0 = time.perf_counter()
                out = call()
                host = time.perf_counter() - t0
                pending = not E.query()
                clones = [t.clone() for t in tensors_of(out)]
                for buf, d in zip(inputs, decoys):
                    buf.copy_(d)
        if misplaced:
            t0 = time.perf_counter()
            out = call()                                     # on the default stream: S has not produced the inputs yet
            host = time.perf_counter() - t0
            clones = [t.clone() for t in tensors_of(out)]
            torch.cuda.default_stream(dev).synchronize()     # the default stream ALONE
            pending = not E.query()
        S.synchronize()
        torch.cuda.synchronize(dev)
    finally:
        if gc_was_on:
            gc.enable()
        torch.cuda.synchronize(dev)
        for buf, r in zip(inputs, reals):
            buf.copy_(r)
        torch.cuda.synchronize(dev)
    return clones, pending, host
