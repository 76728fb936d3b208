"""GPU (MI355X): the stream contract of include/ovn_hip.h ("Conventions"), entry point by entry point, on a NON-default stream.

Every call that takes `void* stream` promises to only enqueue work on that stream, to join whatever it forks back into it, not to make
the host wait unless its comment says so, and to restore the caller's current device.  On the legacy default stream -- the only stream
the rest of the suite ever passes -- none of that can fail: a launch, memset or copy given 0 where `stream` was meant runs in exactly
the right place there.  Here every route is called under `with torch.cuda.stream(S)` behind a delay, with decoys in its input buffers
until S itself copies the real inputs in (tests/_stream_harness.py): work that lands on another stream, or ahead of S, reads decoys and
the result's bits change; a host wait shows as the delay's event having completed when the call returns.

ROWS holds one row per entry point or route: a name, the `ovn_*` functions it reaches, its class and a builder.  The builder gets the
module's engines (`World`) and returns a `Case`: a callable that takes no arguments and reads only device tensors, the input buffers,
and one decoy per buffer (index tensors stay in range, offsets monotone, poses finite: reading a decoy never faults); `probe` replaces
the call in the stream-independence probe where the call itself waits for the whole device.  A row is
`enqueue_only`, or `synchronises` with the sentence of the header / the wrapper's docstring that says so.
tests/test_stream_contract_host.py checks on the CPU that every prototype of the header with a `stream` has a row (or a stated exemption).

Shapes: the smallest case of each module's own reference helper; the main engine is a 64 x 900 depth-only leg (360 columns: spectra and
Delta cache rows exist), the head calls run 9 pairs through chunks of 8, sub-chunks of 3 on two side streams with the yaw head forked."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _stream_harness as H

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

ENQUEUE_ONLY, SYNCHRONISES = "enqueue_only", "synchronises"
Row = collections.namedtuple("Row", "name covers klass reason build")
Case = collections.namedtuple("Case", "call inputs decoys probe", defaults=(None,))
ROWS = []

# prototypes with a `stream` that no row calls, and why
EXEMPT = {
    "ovn_add_leg_layer": "accepted only before ovn_finalize, on a context that has run nothing; its comment says it synchronises `stream`",
    "ovn_gather_scores": "needs a communicator of at least two ranks; tests/test_gpu_two_ranks.py and test_gpu_top_k_two_ranks.py run it",
}

PIPE = dict(chunk_pairs=8, sub_chunk_pairs=3, streams=2, yaw_on_side_stream=True)      # tests/test_gpu_scratch_layout.py's values
SERIAL = dict(chunk_pairs=1024, sub_chunk_pairs=0, streams=1, yaw_on_side_stream=False)
N_PAIRS = 9
NARROW = ((1, 1), False)      # tests/_leg_geometry_ref.py SMALL: the 16 x 131 input whose feature volume is 1 x 45


def row(name, covers, klass=ENQUEUE_ONLY, reason=None):
    def deco(build):
        ROWS.append(Row(name, tuple(covers), klass, reason, build))
        return build
    return deco


# ---- the engines and the inputs several rows share ----------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _volumes(seed, n, width=360):
    """ReLU-like feature volumes: a third of the values zero, one volume with 32 dead channels."""
    rng = np.random.default_rng(seed)
    v = np.maximum(rng.normal(0.3, 1.0, size=(n, width, 128)), 0).astype(np.float32)
    v[1][:, rng.permutation(128)[:32]] = 0
    return v


class World(object):
    """The module's engines and device copies of shared inputs, each made on first use."""

    def __init__(self):
        self.dev = torch.device("cuda", 0)
        self.engines = []
        self.settings = SETTINGS      # engine -> the host-side settings `_settings` last gave it
        self.proven = []              # streams an independence probe has passed: tried first for the next row

    def up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _engine(self, h, w, c, weights, cfg):
        from overlapnet_amd.engine import OvnEngine
        e = OvnEngine(h, w, c, device=0)
        self.engines.append(e)
        e.load_weights(weights, cfg)
        self.settings[e] = {}
        return e

    @functools.cached_property
    def main(self):
        from tools import synthetic as S
        return self._engine(64, 900, 1, S.make_test_weights(1, seed=0), S.REFERENCE_MODEL_CFG)

    def _narrow(self):
        from tests import _leg_geometry_ref as G
        from tests import _leg_grad_ref as L
        e = self._engine(*G.SMALL[NARROW], 4, L.leg_weights(4, G.small_cfg(*NARROW), seed=0, feat_w=45), G.small_cfg(*NARROW))
        assert e.feat_w == 45
        return e

    @functools.cached_property
    def narrow(self):
        return self._narrow()

    @functools.cached_property
    def narrow_rw(self):
        """A second narrow engine for the rows that REPLACE weights: a failure there leaves the other rows' engine alone."""
        return self._narrow()

    @functools.cached_property
    def pool(self):
        """(real, decoy): 10 volumes of 360 columns each -- candidates 0..8, the query 9."""
        return self.up(_volumes(46, N_PAIRS + 1)), self.up(_volumes(47, N_PAIRS + 1))

    @functools.cached_property
    def narrow_case(self):
        from tests import _feature_grad_ref as F
        return F.make_case((45, 15, 5, "idx", "sigmoid"))

    @functools.cached_property
    def narrow_images(self):
        """(real, decoy): 5 scans of the narrow leg's input (one more than a scan block)."""
        from tests import _leg_geometry_ref as G
        from tests import _leg_grad_ref as L
        h, w = G.SMALL[NARROW]
        return tuple(self.up(L.make_images(np.random.default_rng([s, 5]), 5, h, w, 4)) for s in (1, 2))

    @functools.cached_property
    def clouds(self):
        """(points, offsets, max_points, n_points) real and decoy: the six ragged scans of tests/_gt_pairs_ref.py, the decoy with the
        points in reverse order and other (monotone, in-range) offsets."""
        from tests import _gt_pairs_ref as GT
        from tools import synthetic as S
        scans, poses = GT.ragged_scans(S.load_fixture_images())
        pts = np.concatenate(scans)
        off = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int64)
        total = int(off[-1])
        doff = np.array([0, 1000, 1000, 2500, 4000, total - 1, total], np.int64)
        assert len(doff) == len(off) and np.all(np.diff(doff) >= 0) and int(np.diff(doff).max()) <= int(np.diff(off).max())
        dpts = np.ascontiguousarray(pts[::-1] * np.float32(0.5))
        return dict(points=(self.up(pts), self.up(dpts)), offsets=(self.up(off), self.up(doff)), max_points=int(np.diff(off).max()),
                    total=total, n=len(scans), poses=poses)

    def close(self):
        torch.cuda.synchronize()
        for e in self.engines:
            e.close()
        self.settings.clear()

    def streams_for(self, case, count=1):
        """`count` streams that run independently of the default stream and of every stream `case.call` forks onto (the harness's
        probe, with the row's own call as the work on the default stream); proven ones are kept for the rows that follow."""
        found = H.independent_streams(case.probe or case.call, self.dev, count, self.proven)
        self.proven = found + [S for S in self.proven if all(S.cuda_stream != f.cuda_stream for f in found)]
        return found


SETTINGS = {}


def _settings(e, head="f16x3", leg="f16x3", norm="none", split=False, pipe=SERIAL):
    """The engine's host-side settings, each touched only when it changes (none of them takes a stream)."""
    st = SETTINGS[e]
    if st.get("head") != head:
        e.set_head_precision(head)
    if st.get("leg") != leg:
        e.set_leg_precision(leg)
    if st.get("norm") != norm:
        e.set_corr_normalization(norm)
    if st.get("split") != split:
        e.set_head_width_split(split)
    if st.get("pipe") != pipe:
        e.set_head_pipeline(**pipe)
    st.update(head=head, leg=leg, norm=norm, split=split, pipe=pipe)


def _idx(w, a):
    return w.up(np.asarray(a, np.int32))


# ---- leg ------------------------------------------------------------------------------------------------------------------------------
def _main_images(w, n):
    from tests import _leg_grad_ref as L
    return tuple(w.up(L.make_images(np.random.default_rng([s, n]), n, 64, 900, 1)) for s in (3, 4))


def _leg_row(precision, n):
    def build(w):
        e = w.main
        x, dx = _main_images(w, n)

        def call():
            _settings(e, leg=precision)
            return e.leg(x)
        return Case(call, [x], [dx])
    return build


row("leg_f16x3", ["ovn_leg"])(_leg_row("f16x3", 5))          # five scans: the batched strip kernels (more than four)
row("leg_f32", ["ovn_leg"])(_leg_row("f32", 2))


# ---- the heads at 360 columns -----------------------------------------------------------------------------------------------------------
def _heads_row(head="f16x3", spectra=False, dcache=False, indexed=False, pipe=PIPE, norm="none"):
    def build(w):
        e = w.main
        pool, dpool = w.pool
        bufs, decoys = [pool.clone()], [dpool]
        _settings(e, head=head, norm=norm, pipe=pipe)
        spec = dc = None
        if spectra:
            spec = e.spectrum(pool)
            bufs.append(spec)
            decoys.append(e.spectrum(dpool))
        if dcache:
            dc = e.delta_cache(pool)
            bufs.append(dc)
            decoys.append(e.delta_cache(dpool))
        li = ri = None
        if indexed:
            li, ri = _idx(w, [0, 5, 2, 7, 4, 1, 8, 3, 0]), _idx(w, [9, 9, 3, 9, 0, 9, 9, 2, 5])
            bufs += [li, ri]
            decoys += [_idx(w, [1, 6, 3, 8, 5, 2, 0, 4, 1]), _idx(w, [8, 9, 4, 9, 1, 9, 7, 3, 6])]
        p = bufs[0]

        def call():
            _settings(e, head=head, norm=norm, pipe=pipe)
            if indexed:
                return e.heads(p, p, lidx=li, ridx=ri, want_logit=True, want_corr=True, spec_l=spec, spec_r=spec)
            return e.heads(p[:N_PAIRS], p[N_PAIRS:], want_logit=True, want_corr=True, spec_l=None if spec is None else spec[:N_PAIRS],
                           spec_r=None if spec is None else spec[N_PAIRS:], dcache_l=None if dc is None else dc[:N_PAIRS])
        return Case(call, bufs, decoys)
    return build


row("heads", ["ovn_heads"])(_heads_row())
row("heads_spectra", ["ovn_heads_spectral"])(_heads_row(spectra=True))
row("heads_spectra_dcache", ["ovn_heads_spectral"])(_heads_row(spectra=True, dcache=True))
row("heads_indexed", ["ovn_heads"])(_heads_row(indexed=True))
row("heads_spectra_indexed", ["ovn_heads_spectral"])(_heads_row(spectra=True, indexed=True))
row("heads_f32", ["ovn_heads"])(_heads_row(head="f32"))
row("heads_f32_spectra", ["ovn_heads_spectral"])(_heads_row(head="f32", spectra=True))
row("heads_bf16x3", ["ovn_heads"])(_heads_row(head="bf16x3"))
row("heads_bf16x3_spectra", ["ovn_heads_spectral"])(_heads_row(head="bf16x3", spectra=True))
row("heads_euclidean", ["ovn_heads"])(_heads_row(norm="euclidean"))
row("heads_serial_pipeline", ["ovn_heads_spectral"])(_heads_row(spectra=True, dcache=True, pipe=SERIAL))


def _segments_row(spectra, head="f16x3"):
    def build(w):
        e = w.main
        pool, dpool = w.pool
        _settings(e, head=head, pipe=PIPE)
        bufs, decoys = [pool.clone()], [dpool]
        spec = dc = None
        if spectra:
            spec, dc = e.spectrum(pool), e.delta_cache(pool)
            bufs += [spec, dc]
            decoys += [e.spectrum(dpool), e.delta_cache(dpool)]
        cand = _idx(w, [0, 5, 2, 7, 4, 1, 8, 3, 0])
        bufs.append(cand)
        decoys.append(_idx(w, [1, 6, 3, 8, 5, 2, 0, 4, 1]))
        offs, qidx = np.array([0, 4, 4, 9], np.int64), np.array([9, 3, 6], np.int32)       # an empty segment in the middle
        p = bufs[0]

        def call():
            _settings(e, head=head, pipe=PIPE)
            return e.heads_segments(p, p, cand, qidx, offs, spec_pool=spec, spec_q=spec, dcache_pool=dc, want_logit=True, want_corr=True)
        return Case(call, bufs, decoys)
    return build


row("heads_segments", ["ovn_heads_segments"])(_segments_row(True))
row("heads_segments_no_spectra", ["ovn_heads_segments"])(_segments_row(False))
row("heads_segments_f32", ["ovn_heads_segments"])(_segments_row(True, head="f32"))       # the one indexed pass of the other modes


@row("segments_back_to_back", ["ovn_heads_segments", "ovn_top_k_segments"], SYNCHRONISES,
     "ovn_hip.h, ovn_heads_segments: \"a segmented call (this one or ovn_top_k_segments) made while the previous one's table copy is "
     "still pending on its stream waits on the host for that copy\"")
def _segments_back_to_back(w):
    """Two segmented calls with nothing between them: the second rewrites the pinned table the first one's copy still reads."""
    case = _segments_row(True)(w)
    offs = np.array([0, 4, 4, 9], np.int64)

    def call():
        out = case.call()
        return out, w.main.top_k_segments(out["overlap"], offs, out["yaw"], k=3)
    return Case(call, case.inputs, case.decoys)


@row("delta_head", ["ovn_delta_head"])
def _delta_head(w):
    from overlapnet_amd import _lib
    e = w.main
    pool, dpool = w.pool
    p = pool.clone()

    def call():
        _settings(e, pipe=PIPE)
        ov = torch.empty(N_PAIRS, dtype=torch.float32, device=w.dev)
        lg = torch.empty(N_PAIRS, dtype=torch.float32, device=w.dev)
        _lib.check(e.lib.ovn_delta_head(e._h, _ptr(p), None, _ptr(p[N_PAIRS:]), None, N_PAIRS, _ptr(ov), _ptr(lg), e._stream()),
                   "ovn_delta_head")
        return ov, lg
    return Case(call, [p], [dpool])


def _corr_row(spectral, norm="none"):
    def build(w):
        e = w.main
        pool, dpool = w.pool
        _settings(e, norm=norm)
        p, d = (e.spectrum(pool), e.spectrum(dpool)) if spectral else (pool.clone(), dpool)
        li, ri = _idx(w, [0, 5, 2, 7]), _idx(w, [9, 9, 3, 1])

        def call():
            _settings(e, norm=norm)
            f = e.corr_head_spectral if spectral else e.corr_head
            return f(p, p, lidx=li, ridx=ri, want_corr=True), f(p[:N_PAIRS], p[N_PAIRS:], want_corr=True)
        return Case(call, [p, li, ri], [d, _idx(w, [1, 6, 3, 8]), _idx(w, [8, 9, 4, 2])])
    return build


row("corr_head", ["ovn_corr_head"])(_corr_row(False))
row("corr_head_standardization", ["ovn_corr_head"])(_corr_row(False, norm="standardization"))
row("corr_head_spectral", ["ovn_corr_head_spectral"])(_corr_row(True))


def _volume_row(method, covers, head="f16x3", norm="none"):
    def build(w):
        e = w.main
        pool, dpool = w.pool
        p = pool.clone()

        def call():
            _settings(e, head=head, norm=norm)
            if method == "delta_cache":      # a row ends in 60 floats of padding that nothing writes or reads: zeroed, so that bits compare
                return e.delta_cache(p, out=torch.zeros((p.shape[0], e.DELTA_CACHE_ELEMS), dtype=torch.float32, device=w.dev))
            return getattr(e, method)(p)
        return Case(call, [p], [dpool])
    return row("%s%s%s" % (method, "" if head == "f16x3" else "_" + head, "" if norm == "none" else "_" + norm), covers)(build)


_volume_row("spectrum", ["ovn_spectrum"])
_volume_row("spectrum", ["ovn_spectrum"], head="f32", norm="scaling")          # the path through norm_buf, fp32 DFT
_volume_row("spectrum", ["ovn_spectrum"], norm="euclidean")
_volume_row("delta_cache", ["ovn_delta_cache"])


@row("head_walk_stats", ["ovn_head_walk_stats"], SYNCHRONISES,
     "ovn_hip.h, ovn_head_walk_stats: \"Synchronises `stream`.\"")
def _walk_stats(w):
    e = w.main
    pool, dpool = w.pool
    p = pool.clone()

    def call():
        _settings(e, pipe=PIPE)
        out = e.heads(p[:N_PAIRS], p[N_PAIRS:])
        st = e.head_walk_stats()
        return out, torch.tensor([st["max_slices"], st["live_channels"], int(st["compacted"])] + st["slices_per_group_pair"],
                                 dtype=torch.int32).to(w.dev)
    dp = dpool.clone()
    dp[N_PAIRS][:, :64] = 0             # the decoy query has other live channels: the statistics differ too
    return Case(call, [p], [dp])


# ---- the heads at another width (the narrow leg: 45 columns) ------------------------------------------------------------------------------
def _narrow_pool(w):
    c = w.narrow_case
    return w.up(c["pool"]), w.up(np.ascontiguousarray(c["pool"][::-1] * np.float32(0.5)))


def _narrow_heads_row(head, split):
    def build(w):
        e = w.narrow
        c = w.narrow_case
        p, d = _narrow_pool(w)
        li, ri = _idx(w, c["lidx"]), _idx(w, c["ridx"])
        k = p.shape[0]

        def call():
            _settings(e, head=head, split=split, pipe=dict(PIPE, chunk_pairs=4))
            return e.heads(p, p, lidx=li, ridx=ri, want_logit=True, want_corr=True), e.heads(p, p[1:2], want_logit=True)
        return Case(call, [p, li, ri], [d, _idx(w, [(v + 1) % k for v in c["lidx"]]), _idx(w, [(v + 2) % k for v in c["ridx"]])])
    return build


row("narrow_heads_f32", ["ovn_heads"])(_narrow_heads_row("f32", False))
row("narrow_heads_f16x3", ["ovn_heads"])(_narrow_heads_row("f16x3", False))
row("narrow_heads_bf16x3", ["ovn_heads"])(_narrow_heads_row("bf16x3", False))
row("narrow_heads_width_split", ["ovn_heads"])(_narrow_heads_row("f16x3", True))


@row("narrow_heads_segments_width_split", ["ovn_heads_segments"])
def _narrow_segments(w):
    e = w.narrow
    p, d = _narrow_pool(w)
    k = p.shape[0]
    cand = _idx(w, [0, 1, 2, 3, 4, 0, 2])
    offs, qidx = np.array([0, 3, 3, 7], np.int64), np.array([1, 0, 4], np.int32)

    def call():
        _settings(e, split=True, pipe=dict(PIPE, chunk_pairs=4))
        return e.heads_segments(p, p, cand, qidx, offs, want_logit=True, want_corr=True)
    return Case(call, [p, cand], [d, _idx(w, [(v + 1) % k for v in [0, 1, 2, 3, 4, 0, 2]])])


@row("debug_head_activations", ["ovn_heads", "ovn_debug_head_activations"])
def _head_activations(w):
    e = w.narrow
    p, d = _narrow_pool(w)

    def call():
        _settings(e, head="f32")                       # the serial pipeline: the call runs as one chunk, which the hook needs
        out = e.heads(p, p[1:2], want_logit=True)
        return out, e.debug_head_activations(int(p.shape[0]))
    return Case(call, [p], [d])


# ---- training ---------------------------------------------------------------------------------------------------------------------------
@row("delta_head_grad", ["ovn_delta_head_grad"])
def _delta_head_grad(w):
    e = w.narrow
    c = w.narrow_case
    p, d = _narrow_pool(w)
    li, ri, t = _idx(w, c["lidx"]), _idx(w, c["ridx"]), w.up(c["targets"])
    k = p.shape[0]

    def call():
        _settings(e, pipe=dict(SERIAL, chunk_pairs=4))             # two chunks of whole pair blocks
        r = e.delta_head_grad(p, p, t, lidx=li, ridx=ri, loss="sigmoid", scale=5.0, want_activations=True)
        return r["flat"], r["loss"], r["overlap"], r["o2"], r["o3"]
    return Case(call, [p, li, ri, t], [d, _idx(w, [(v + 1) % k for v in c["lidx"]]), _idx(w, [(v + 2) % k for v in c["ridx"]]),
                                       w.up(1.0 - c["targets"])])


@row("heads_feature_grad", ["ovn_heads_feature_grad"])
def _heads_feature_grad(w):
    e = w.narrow
    c = w.narrow_case
    p, d = _narrow_pool(w)
    li, ri, t, b = _idx(w, c["lidx"]), _idx(w, c["ridx"]), w.up(c["targets"]), _idx(w, c["bins"])
    k = p.shape[0]

    def call():
        _settings(e, pipe=dict(SERIAL, chunk_pairs=4))
        r = e.heads_feature_grad(p, p, t, b, lidx=li, ridx=ri, loss="sigmoid", want_head_grads=True)
        return r["dfeat_l"], r["dfeat_r"], r["loss"], r["overlap"], r["corr"], r["flat"]
    return Case(call, [p, li, ri, t, b],
                [d, _idx(w, [(v + 1) % k for v in c["lidx"]]), _idx(w, [(v + 2) % k for v in c["ridx"]]), w.up(1.0 - c["targets"]),
                 _idx(w, [(int(v) + 7) % 45 for v in c["bins"]])])


@row("leg_forward_train", ["ovn_leg_forward_train"])
def _leg_forward_train(w):
    e = w.narrow
    x, dx = w.narrow_images

    def call():
        _settings(e)
        return e.leg_forward_train(x)
    return Case(call, [x], [dx])


def _whole_buffer(acts):
    """The one layer-major buffer the activations of `leg_forward_train` are views of, as a flat tensor on the same storage."""
    n = sum(t.numel() for t in acts)
    flat = torch.empty(0, dtype=torch.float32, device=acts[0].device).set_(acts[0].untyped_storage(), acts[0].storage_offset(), (n,))
    assert flat.data_ptr() == acts[0].data_ptr() and acts[-1].data_ptr() + 4 * acts[-1].numel() == flat.data_ptr() + 4 * n
    return flat


@row("leg_backward", ["ovn_leg_backward"])
def _leg_backward(w):
    e = w.narrow
    x, dx = (t.clone() for t in w.narrow_images)
    _settings(e)
    acts, dacts = e.leg_forward_train(x), e.leg_forward_train(dx)
    flat, dflat = _whole_buffer(acts), _whole_buffer(dacts)
    rng = np.random.default_rng(8)
    g, dg = (w.up(rng.normal(0.0, 1.0, tuple(acts[-1].shape[:1]) + (45, 128)).astype(np.float32)) for _ in range(2))

    def call():
        _settings(e)
        return e.leg_backward(x, acts, g, slice_scans=4)["flat"]             # two slices: 4 + 1 scans
    return Case(call, [x, flat, g], [dx, dflat, dg])


@row("debug_conv", ["ovn_debug_conv"])
def _debug_conv(w):
    e = w.narrow
    x, dx = w.narrow_images

    def call():
        _settings(e)
        first = e.debug_conv(0, x)
        _settings(e, leg="f32")
        return first, e.debug_conv(0, x)
    return Case(call, [x], [dx])


@row("debug_conv_grad", ["ovn_debug_conv_grad"])
def _debug_conv_grad(w):
    e = w.narrow
    x, dx = (t.clone() for t in w.narrow_images)
    _settings(e)
    a0, a1 = (t.clone() for t in e.leg_forward_train(x)[:2])
    d0, d1 = (t.clone() for t in e.leg_forward_train(dx)[:2])
    rng = np.random.default_rng(9)
    g0, dg0 = (w.up(rng.normal(0.0, 1.0, tuple(a0.shape)).astype(np.float32)) for _ in range(2))
    g1, dg1 = (w.up(rng.normal(0.0, 1.0, tuple(a1.shape)).astype(np.float32)) for _ in range(2))

    def call():
        _settings(e)
        first = e.debug_conv_grad(0, x, a0, g0)              # cin = 4: the plain fp64 data gradient
        return first, e.debug_conv_grad(1, a0, a1, g1)       # cin a multiple of 16: the MFMA one
    return Case(call, [x, a0, a1, g0, g1], [dx, d0, d1, dg0, dg1])


@row("grad_reduce_adagrad", ["ovn_grad_reduce_adagrad"])
def _grad_reduce(w):
    from tests import _grad_reduce_ref as GR
    e = w.narrow
    weights = GR.WEIGHT_SETS[3][1]                            # a rank with weight 0: its NaN row must not be read
    c, d = (GR.make_case(1027, 1032, 3, weights, seed=s) for s in (0, 1))
    g, p, a = w.up(c["grads"]), w.up(c["params"]), w.up(c["accum"])

    def call():
        out = e.grad_reduce_adagrad(g, weights, p, a, lr=0.01, eps=1e-7, want_grad=True)       # p, a: updated in place
        return p, a, out, e.grad_reduce_adagrad(g, weights, count=1001)
    return Case(call, [g, p, a], [w.up(d["grads"]), w.up(d["params"]), w.up(d["accum"])])


@row("set_head_weights", ["ovn_set_head_weights"], SYNCHRONISES,
     "ovn_hip.h, ovn_add_leg_layer / ovn_set_head_weights: \"the caller may release its buffers after the call returns (the call "
     "synchronises `stream`)\", \"Same ownership rule as above.\"")
def _set_head_weights(w):
    e = w.narrow_rw
    p, _ = _narrow_pool(w)
    wts = _narrow_weights(w)
    params = [w.up(wts[k]) for k in e.HEAD_PARAMS]
    li, ri = _idx(w, w.narrow_case["lidx"]), _idx(w, w.narrow_case["ridx"])

    def heads():
        _settings(e)
        return e.heads(p, p, lidx=li, ridx=ri, want_logit=True)

    def call():
        e.set_head_weights(params)
        return heads()
    # replacing weights frees the library's old copies, and hipFree waits for the whole device, a probe's delay included: the probe
    # runs the part of the call that launches
    return Case(call, params, [t * 0.75 for t in params], heads)


def _narrow_weights(w):
    from tests import _leg_geometry_ref as G
    from tests import _leg_grad_ref as L
    return L.leg_weights(4, G.small_cfg(*NARROW), seed=0, feat_w=45)


@row("set_leg_weights", ["ovn_set_leg_layer_weights"], SYNCHRONISES,
     "ovn_hip.h, ovn_set_leg_layer_weights: \"Synchronises `stream`.\"")
def _set_leg_weights(w):
    e = w.narrow_rw
    x, _ = w.narrow_images
    wts = _narrow_weights(w)
    params = [w.up(wts[k]) for k in e.leg_param_names()]

    def leg():
        _settings(e)
        return e.leg(x)

    def call():
        e.set_leg_weights(params)
        return leg()
    return Case(call, params, [t * 0.75 for t in params], leg)      # (as set_head_weights: hipFree waits for the device)


# ---- the decision kernels -----------------------------------------------------------------------------------------------------------------
def _scores(w, n, seed):
    rng = np.random.default_rng(seed)
    ov = rng.uniform(0, 1, n).astype(np.float32)
    ov[::97] = np.nan
    ov[5] = ov[1100] = 0.995                                                    # a tie: the first one wins
    return w.up(ov), _idx(w, rng.integers(-179, 181, n)), _idx(w, rng.permutation(n) + 10)


def _decision_row(name, covers, fn, klass=ENQUEUE_ONLY, reason=None):
    def build(w):
        e = w.main
        ov, yaw, ids = _scores(w, 1500, 0)
        return Case(lambda: fn(w, e, ov, yaw, ids), [ov, yaw, ids], list(_scores(w, 1500, 1)))
    row(name, covers, klass, reason)(build)


_decision_row("best_match", ["ovn_best_match"], lambda w, e, ov, yaw, ids: e.best_match(ov, yaw, 0.3, ids=ids))
_decision_row("best_match_host", ["ovn_best_match"],
              lambda w, e, ov, yaw, ids: torch.from_numpy(e.best_match(ov, yaw, 0.3, ids=ids, host=True)).to(w.dev), SYNCHRONISES,
              "OvnEngine.best_match: \"host=True: the kernel writes the record straight into pinned host memory (device-visible at the "
              "same address) and the call waits for the stream\"")
_decision_row("top_k", ["ovn_top_k"], lambda w, e, ov, yaw, ids: (e.top_k(ov, yaw, k=5, ids=ids), e.top_k(ov, None, k=1024, index_offset=7)))
_decision_row("top_k_segments", ["ovn_top_k_segments"],
              lambda w, e, ov, yaw, ids: e.top_k_segments(ov, np.array([0, 700, 700, 1500], np.int64), yaw, k=5, ids=ids))


# ---- preprocessing and ground truth ------------------------------------------------------------------------------------------------------
ALL_IMAGES = ("range", "vertex", "intensity", "idx", "normal")


@row("project", ["ovn_project"])
def _project(w):
    e, c = w.main, w.clouds
    pts, off = c["points"][0].clone(), c["offsets"][0].clone()

    def call():
        return e.project(pts, off, c["max_points"], want=ALL_IMAGES, stacked_flags=(True, True, True))
    return Case(call, [pts, off], [c["points"][1], c["offsets"][1]])


@row("project_probs", ["ovn_project_semantic"])
def _project_probs(w):
    e, c = w.main, w.clouds
    pts, off = c["points"][0].clone(), c["offsets"][0].clone()
    rng = np.random.default_rng(20)
    probs, dprobs = (w.up(rng.dirichlet(np.ones(20), c["total"]).astype(np.float32)) for _ in range(2))

    def call():
        return e.project(pts, off, c["max_points"], want=ALL_IMAGES + ("semantic", "sem_idx"), stacked_flags=(True, True, True, True),
                         probs=probs, n_classes=20, n_points=c["total"])
    return Case(call, [pts, off, probs], [c["points"][1], c["offsets"][1], dprobs])


@row("normals", ["ovn_normals"])
def _normals(w):
    e, c = w.main, w.clouds
    r, d = (e.project(c["points"][i], c["offsets"][i], c["max_points"], want=("range", "vertex")) for i in (0, 1))
    rng, vtx = r["range"], r["vertex"]
    return Case(lambda: e.normals(rng, vtx), [rng, vtx], [d["range"], d["vertex"]])


@row("projection_angles", ["ovn_projection_angles"])
def _projection_angles(w):
    e, c = w.main, w.clouds
    pts = c["points"][0].clone()
    return Case(lambda: e.projection_angles(pts), [pts], [c["points"][1]])


def _poses_dev(w, poses):
    return w.up(np.asarray(poses, np.float64))


@row("gt_range_images", ["ovn_gt_range_images"])
def _gt_range_images(w):
    e, c = w.main, w.clouds
    pts, off = c["points"][0].clone(), c["offsets"][0].clone()
    ref, dref = _poses_dev(w, c["poses"]), _poses_dev(w, c["poses"][::-1])
    inv, dinv = _poses_dev(w, np.linalg.inv(c["poses"][2])), _poses_dev(w, np.linalg.inv(c["poses"][4]))

    def call():
        return e.gt_range_images(pts, off, c["max_points"], ref, inv), e.gt_range_images(pts, off, c["max_points"])
    return Case(call, [pts, off, ref, inv], [c["points"][1], c["offsets"][1], dref, dinv])


@row("gt_overlap_counts", ["ovn_gt_overlap_counts"])
def _gt_overlap_counts(w):
    e, c = w.main, w.clouds
    imgs, dimgs = (e.gt_range_images(c["points"][i], c["offsets"][i], c["max_points"]) for i in (0, 1))
    cur, dcur = imgs[0:1].clone(), dimgs[4:5].clone()
    return Case(lambda: e.gt_overlap_counts(imgs, cur), [imgs, cur], [dimgs, dcur])


@row("gt_pair_counts", ["ovn_gt_pair_counts"])
def _gt_pair_counts(w):
    e, c = w.main, w.clouds
    pts, off = c["points"][0].clone(), c["offsets"][0].clone()
    inv_np = np.stack([np.linalg.inv(p) for p in c["poses"]])
    poses, inv = _poses_dev(w, c["poses"]), _poses_dev(w, inv_np)
    cur, dcur = (e.gt_range_images(c["points"][i], c["offsets"][i], c["max_points"]) for i in (0, 1))
    fi, ri = _idx(w, [4, 0, 4]), _idx(w, [5, 5, 2, 0])

    def call():
        return e.gt_pair_counts(pts, off, poses, inv, cur, fi, ri), e.gt_pair_counts(pts, off, poses, inv, cur)
    return Case(call, [pts, off, poses, inv, cur, fi, ri],
                [c["points"][1], c["offsets"][1], _poses_dev(w, c["poses"][::-1]), _poses_dev(w, inv_np[::-1]), dcur, _idx(w, [0, 5, 3]),
                 _idx(w, [4, 0, 5, 2])])


# ---- map building, verification, localization -----------------------------------------------------------------------------------------
@row("render_scans", ["ovn_render_scans"])
def _render_scans(w):
    from overlapnet_amd.mesh import TriangleMesh
    from tests import _render_ref as R
    e = w.main
    mesh = TriangleMesh(*R.scene(0))
    md = mesh.device(e, with_bvh=True)
    all_poses = R.scene_poses(6)
    poses, dposes = _poses_dev(w, all_poses[:3]), _poses_dev(w, all_poses[3:])
    verts = md["vertices"]
    dverts = (verts * 0.98).contiguous()              # every index stays valid; the boxes of the hierarchy no longer fit, which only
    sensor = dict(fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)      # changes what a decoy run returns

    def call():
        a = e.render_scans(mesh, poses, 16, 90, want=("range", "tri_id", "vertex", "normal"), stacked_flags=(True, True), **sensor)
        return a, e.render_scans(mesh, poses, 16, 90, want=("range", "tri_id"), exhaustive=True, **sensor)
    return Case(call, [poses, verts], [dposes, dverts])


@row("tsdf_integrate", ["ovn_tsdf_integrate"])
def _tsdf_integrate(w):
    from tests import _render_ref as R
    from tests import _tsdf_ref as T
    e = w.main
    name = "70x5x3"
    shape, _, (h, wd) = T.CASES_FUSED[name]
    origin = T._origins()[name]
    ranges, poses = T.scans(h, wd)
    t0, w0 = T.fresh(shape)
    tsdf, weight, rng, ps = w.up(t0), w.up(w0), w.up(ranges), _poses_dev(w, poses)
    decoys = [torch.full_like(tsdf, 0.25), torch.full_like(weight, 2.0), w.up(np.ascontiguousarray(ranges[::-1, :, ::-1])),
              _poses_dev(w, poses[::-1])]

    def call():
        e.tsdf_integrate(tsdf, weight, origin, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, rng, ps, R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE)
        return tsdf, weight                               # updated in place
    return Case(call, [tsdf, weight, rng, ps], decoys)


def _plane_volumes(w):
    from tests import _tsdf_ref as T
    d, wt, origin, voxel, _ = T.plane_volume()
    w2 = wt.copy()
    w2[3, 4, 5] = 0.5                                   # the decoy: an unseen sample and the surface on the other side
    return w.up(d), w.up(wt), w.up(-d - np.float32(0.3)), w.up(w2), origin, voxel


@row("tsdf_triangles", ["ovn_tsdf_triangles"], SYNCHRONISES,
     "OvnEngine.tsdf_triangles: \"Returns (triangles (min(T, capacity),3,3) device tensor or None, T)\" -- T is a host integer, read "
     "back after every call of ovn_tsdf_triangles")
def _tsdf_triangles(w):
    e = w.main
    d, wt, dd, dw, origin, voxel = _plane_volumes(w)

    def call():
        tri, total = e.tsdf_triangles(d, wt, origin, voxel)
        return tri, torch.tensor([total], dtype=torch.int64).to(w.dev)
    return Case(call, [d, wt], [dd, dw])


@row("tsdf_triangles_device_count", ["ovn_tsdf_triangles"])
def _tsdf_triangles_device(w):
    """The entry point itself, as ovn_hip.h states it: the count stays on the device."""
    from overlapnet_amd import _lib
    e = w.main
    d, wt, dd, dw, origin, voxel = _plane_volumes(w)
    nz, ny, nx = (int(v) for v in d.shape)
    org = (C.c_double * 3)(*[float(v) for v in origin])
    cap = 4096

    def call():
        tri = torch.zeros((cap, 3, 3), dtype=torch.float32, device=w.dev)
        count = torch.zeros(1, dtype=torch.int64, device=w.dev)
        _lib.check(e.lib.ovn_tsdf_triangles(e._h, _ptr(d), _ptr(wt), nx, ny, nz, org, float(voxel), 1.0, _ptr(tri), cap, _ptr(count),
                                            e._stream()), "ovn_tsdf_triangles")
        return tri, count
    return Case(call, [d, wt], [dd, dw])


@row("icp_register", ["ovn_icp_register"])
def _icp_register(w):
    from tests import _icp_ref as I
    e = w.main
    h, wd = I.ROOM_SHAPES[1]
    tgt, src, _, t0 = I.room_pair(I.ROOM_CASES[0], n_rays=4000)
    other = I.room_pair(I.ROOM_CASES[2], n_rays=4000)[1]
    pts = np.concatenate([tgt, src, other])
    off = w.up(np.array([0, len(tgt), len(tgt) + len(src), len(pts)], np.int64))
    m = e.project(w.up(pts), off, 4000, proj_h=h, proj_w=wd, want=("range", "vertex", "normal"))
    vtx, nrm, rng = m["vertex"], m["normal"], m["range"]
    si, ti = _idx(w, [1, 2, 0]), _idx(w, [0, 0, 1])
    init = _poses_dev(w, np.stack([t0, I.rz(1.0), np.linalg.inv(t0)]))

    def call():
        return e.icp_register(vtx, nrm, rng, si, ti, init, iterations=4, min_inliers=16, want_system=True)
    return Case(call, [vtx, nrm, rng, si, ti, init],
                [vtx.flip(0).contiguous(), nrm.flip(0).contiguous(), rng.flip(0).contiguous(), _idx(w, [2, 0, 1]), _idx(w, [1, 2, 2]),
                 _poses_dev(w, np.stack([np.eye(4), t0, I.rz(-3.0)]))])


MCL_GRID = dict(origin=(-3.5, -2.5), resolution=1.0, nx=7, ny=5, n_frames=9)          # the 7 x 5 grid with holes of tests/test_gpu_mcl.py
MCL_P = 1025                                                                          # one particle past a workgroup of 1024


def _mcl_table(seed):
    t = np.random.default_rng(seed).integers(0, 9, 35).astype(np.int32)
    t[[0, 6, 12, 17, 23, 34]] = -1
    return t


@row("mcl_predict", ["ovn_mcl_predict"])
def _mcl_predict(w):
    from tests import _mcl_ref as M
    e = w.main
    parts = M.predict_case(MCL_P)
    parts[:, :2] *= 0.1                                  # within a few metres: most particles land on the grid
    p, table = w.up(parts), w.up(_mcl_table(5))
    ar = torch.arange(MCL_GRID["n_frames"], dtype=torch.int32, device=w.dev)

    def call():
        pf, slot, lst, rec = e.mcl_predict(p, M.PREDICT_ODOM, M.PREDICT_SIGMA, M.PREDICT_SEED, M.PREDICT_STEP, table, **MCL_GRID)
        return p, pf, slot, torch.where(ar < rec[0], lst, torch.full_like(lst, -1)), rec       # only the first U list entries are written
    return Case(call, [p, table], [w.up(np.ascontiguousarray(parts[::-1] * np.float32(0.5))), w.up(_mcl_table(6))])


def _mcl_update_inputs(w, P):
    from tests import _mcl_ref as M
    c, d = M.update_case(P), M.update_case(P + 1)
    keys = ("particles", "particle_frame", "frame_slot", "frame_yaw", "overlap", "yaw")
    u = min(len(c["overlap"]), len(d["overlap"]))
    real = [w.up(c[k][:u] if k in ("overlap", "yaw") else c[k]) for k in keys]
    decoy = [w.up(d[k][:u] if k in ("overlap", "yaw") else (d[k][:P] if k in ("particles", "particle_frame") else d[k])) for k in keys]
    return real, decoy                                  # a slot beyond the u scores counts as off the map: no decoy index is out of range


@row("mcl_update", ["ovn_mcl_update"])
def _mcl_update(w):
    from tests import _mcl_ref as M
    e = w.main
    real, decoy = _mcl_update_inputs(w, MCL_P)
    p, pf, slot, fyaw, ov, yaw = real

    def call():
        est, spread = e.mcl_update(p, pf, slot, fyaw, ov, yaw, want_spread=True, **M.UPDATE_OBS)
        return p, est, spread
    return Case(call, real, decoy)


@row("mcl_resample", ["ovn_mcl_resample"])
def _mcl_resample(w):
    from tests import _mcl_ref as M
    e = w.main
    p, d = w.up(M.update_case(MCL_P)["particles"]), w.up(M.update_case(MCL_P + 1)["particles"][:MCL_P])

    def call():
        return e.mcl_resample(p, M.PREDICT_SEED, 3), e.mcl_resample(p, M.PREDICT_SEED, 4, n_out=2500)
    return Case(call, [p], [d])


ROW_IDS = [r.name for r in ROWS]
BY_NAME = {r.name: r for r in ROWS}


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    torch.cuda.set_device(0)
    w = World()
    mode, per = H.calibrate(w.dev)
    print("delay of %.3f s asked for, %.3f s measured (%s)" % (H.TARGET_DELAY_S, H.measured_delay(H.TARGET_DELAY_S, w.dev), mode))
    yield w
    w.close()


@pytest.fixture(scope="module")
def prepared(world):
    """name -> the row's case with its default-stream results: the warm-up, `expected`, `expected_decoy`, the warm host time."""
    made = {}

    def get(name):
        if name not in made:
            case = BY_NAME[name].build(world)
            reals = [b.clone() for b in case.inputs]
            torch.cuda.synchronize()
            H.run_plain(case.call, case.inputs, reals)                              # warm-up: every context-owned buffer reaches its size
            torch.cuda.synchronize()
            expected, host = H.run_plain(case.call, case.inputs, reals)
            torch.cuda.synchronize()
            expected_decoy, _ = H.run_plain(case.call, case.inputs, case.decoys)
            torch.cuda.synchronize()
            for b, r in zip(case.inputs, reals):
                b.copy_(r)
            torch.cuda.synchronize()
            made[name] = dict(case=case, expected=expected, expected_decoy=expected_decoy, host=host, reals=reals)
        return made[name]
    return get


def _assert_has_power(name, p):
    assert len(p["expected"]) > 0, "%s returns nothing to compare" % name
    assert not H.same_bits(p["expected"], p["expected_decoy"]), "%s: the decoys give the real inputs' result, the row can detect nothing" % name


@pytest.mark.parametrize("name", ROW_IDS)
def test_call_is_ordered_on_its_stream(name, world, prepared):
    r, p = BY_NAME[name], prepared(name)
    case = p["case"]
    _assert_has_power(name, p)
    for b, v in zip(case.inputs, p["reals"]):
        b.copy_(v)
    S, = world.streams_for(case)                            # asserts: S shares no hardware queue with the default stream or the call's side streams
    with torch.cuda.stream(S):                              # once on S without a delay: torch's allocator gets its blocks for this stream
        H.run_plain(case.call, case.inputs, p["reals"])
    torch.cuda.synchronize()
    delay = H.case_delay(p["host"])
    got, pending, host = H.run_delayed(case.call, case.inputs, case.decoys, p["reals"], delay_s=delay, stream=S)
    print("STREAM %s: class %s, delay %.3f s, warm host time %.6f s, host time behind the delay %.6f s, delay pending at return: %s "
          "(stream %#x, proven independent)" % (name, r.klass, delay, p["host"], host, pending, S.cuda_stream))
    assert len(got) == len(p["expected"])
    for i, (a, b) in enumerate(zip(got, p["expected"])):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, i)
        same = torch.equal(H.bits(a), H.bits(b))
        decoy = (not same) and torch.equal(H.bits(a), H.bits(p["expected_decoy"][i]))
        assert same, "%s: output %d differs from the default-stream bits%s" % (name, i, " and equals the DECOY's result" if decoy else "")
    if r.klass == ENQUEUE_ONLY:
        assert pending, ("%s made the host wait: the delay (%.3f s) had completed when the call returned after %.3f s%s"
                         % (name, delay, host, "" if host >= 0.5 * delay else " -- the call returned quickly, so the delay was too short"))


@pytest.mark.parametrize("name", ["spectrum", "heads_spectra_dcache", "project"])
def test_the_harness_sees_a_misplaced_call(name, world, prepared):
    """The same delayed input production on S, but the call goes to the default stream: it must read the decoys, and S must still be
    inside its delay once the default stream has drained -- torch's streams do not order against the null stream, the scheme has power."""
    p = prepared(name)
    case = p["case"]
    _assert_has_power(name, p)
    for b, v in zip(case.inputs, p["reals"]):
        b.copy_(v)
    S, = world.streams_for(case)
    got, pending, host = H.run_delayed(case.call, case.inputs, case.decoys, p["reals"], delay_s=H.case_delay(p["host"]), stream=S,
                                       misplaced=True)
    assert pending, "the side stream's delay was over when the default stream had drained"
    assert H.same_bits(got, p["expected_decoy"]), "a call on the default stream did not read the decoys"
    assert not H.same_bits(got, p["expected"])


@pytest.mark.parametrize("name", ["heads_spectra_dcache", "heads_segments"])
def test_two_streams_in_turn(name, world, prepared):
    """One context, two caller streams one after the other (the header allows one stream at a time): the fork / join events and the
    segment table's events survive the change of stream."""
    p = prepared(name)
    case = p["case"]
    for b, v in zip(case.inputs, p["reals"]):
        b.copy_(v)
    S1, S2 = world.streams_for(case, 2)                     # both independent of the default stream and of the context's side streams
    for S in (S1, S2):                                      # the allocator's blocks for both streams
        with torch.cuda.stream(S):
            H.run_plain(case.call, case.inputs, p["reals"])
        torch.cuda.synchronize()                            # one stream at a time: calls of one context share its scratch
    with torch.cuda.stream(S1):
        H.enqueue_delay(H.TARGET_DELAY_S, world.dev)
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
def test_caller_device_is_restored(world, prepared):
    cases = {name: prepared(name) for name in ("leg_f16x3", "heads_spectra_dcache", "project", "top_k", "mcl_update")}
    torch.cuda.synchronize()
    try:
        torch.cuda.set_device(1)
        for name, p in cases.items():
            got, _ = H.run_plain(p["case"].call, p["case"].inputs, p["reals"])
            assert torch.cuda.current_device() == 1, "%s left device %d current" % (name, torch.cuda.current_device())
            torch.cuda.synchronize(world.dev)
            assert H.same_bits(got, p["expected"]), name
    finally:
        torch.cuda.set_device(0)
