"""Thin host wrapper around one libovn_hip context (one per GPU per process).

PyTorch-ROCm is used only as the owner of device memory and for the current HIP stream; every
computation is a C-ABI call into the hand-written HIP kernels.  Nothing here falls back to torch
math or to the CPU oracle.

Every entry point is built from the same three pieces: `OvnEngine._check` refuses a tensor the library must not see, `_call` makes
the native call on this engine's device and raises on its status, and `_image_outputs` allocates the per-pixel outputs of the calls
that make images.  A new entry point is a row in `_lib.SIGNATURES`, a list of checks and one `_call`.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import weights as W

FEAT_W = 360         # the reference's leg output width; an engine's own width is OvnEngine.feat_w (weights.feature_width)
FEAT_C = 128
SEMANTIC_CLASSES_MAX = 64   # OVN_SEMANTIC_CLASSES_MAX of include/ovn_hip.h


class _NoContext(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_CONTEXT = _NoContext()
_MATCH_PENDING = 0x7FFFFFF0      # word 3 of a best-match record that the kernel has not written yet (it writes 0 or 1)
_F32, _I32 = torch.float32, torch.int32
# per-pixel outputs of the calls that make images, in the order the library takes them: name -> (trailing shape, dtype)
_PROJECT_OUTPUTS = {"range": ((), _F32), "vertex": ((4,), _F32), "intensity": ((), _F32), "idx": ((), _I32), "normal": ((3,), _F32)}
_RENDER_OUTPUTS = {"range": ((), _F32), "tri_id": ((), _I32), "vertex": ((4,), _F32), "normal": ((3,), _F32)}
_RAYCAST_OUTPUTS = {"range": ((), _F32), "vertex": ((4,), _F32), "normal": ((3,), _F32)}


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else C.c_void_p(t.data_ptr())


def _require_gpu() -> None:
    if not torch.cuda.is_available():
        raise _lib.OvnError("no HIP device visible: overlapnet_amd runs on MI355X (gfx950) only, there is no CPU path")


class OvnEngine:
    """Owns the native context + device copies of nothing but the library's own re-tiled weights."""

    def __init__(self, in_h: int = 64, in_w: int = 900, in_c: int = 4, device: Optional[int] = None):
        _require_gpu()
        self.lib = _lib.load()
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.in_h, self.in_w, self.in_c = int(in_h), int(in_w), int(in_c)
        h = C.c_void_p()
        with self._dev():
            _lib.check(self.lib.ovn_create(self.device_index, self.in_h, self.in_w, self.in_c, C.byref(h)), "ovn_create")
        self._h = h
        self.feat_w = 0
        self._leg_ready = False
        self._head_ready = False
        self.head_precision = "f16x3"
        self.head_width_split = False
        self.leg_precision = "f16x3"
        self.projection_trig = "numpy_avx512"
        self.head_compaction = True
        self.negate_diffs = False            # deltaLayer_negateDiffs of the registered weights (load_weights)
        self.conv1size = 15
        self._leg_cfg: dict = {}             # the model keys the registered leg was built from (load_weights)
        self.check_device_indices = False    # opt-in range check of pair-index tensors that already live on the device (_idx)
        self._render_tables: dict = {}       # render_scans: the device ray tables of the last sensor geometry

    # -- lifetime -----------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            with self._dev():   # the C side restores the caller's device too; belt and braces
                self.lib.ovn_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self):
        """Context that makes this engine's GPU torch's current device -- a no-op when it already is (the library selects its context's
        device itself; what needs the torch side are allocations and streams, and switching costs microseconds per call on the chain
        of a single query)."""
        return _NO_CONTEXT if torch.cuda.current_device() == self.device_index else torch.cuda.device(self.device)

    # -- the pieces every entry point is made of ------------------------------------------------------
    def _call(self, name: str, *args, what: Optional[str] = None) -> None:
        """The native call `name(ctx, *args)` with this engine's GPU current; a status other than 0 raises with the library's message.
        The stream is among `args`: second in the newer entry points, last in the older ones."""
        with self._dev():
            _lib.check(getattr(self.lib, name)(self._h, *args), what or name)

    def _check(self, t: Optional[torch.Tensor], what: str, dtype=_F32, shape=None, numel: Optional[int] = None,
               ndim: Optional[int] = None, optional: bool = False, pinned_ok: bool = False) -> Optional[torch.Tensor]:
        """The one test of a tensor that goes to the library: contiguous, of `dtype`, on this device (pinned_ok: or pinned host memory,
        which the device sees at the same address), and of the exact `shape`, `numel` elements or `ndim` dimensions where given.
        `what` names the argument in the message, with the call in front ("call: name") where one is named.  Returns the tensor."""
        if t is None and optional:
            return None
        if (t is None or t.dtype != dtype or not t.is_contiguous()
                or not (t.device == self.device or (pinned_ok and t.device.type == "cpu" and t.is_pinned()))
                or (shape is not None and tuple(t.shape) != tuple(shape)) or (numel is not None and t.numel() != numel)
                or (ndim is not None and t.dim() != ndim)):
            size = ("" if shape is None else " of shape %s" % (tuple(shape),)) + ("" if numel is None else " of %d elements" % numel) \
                + ("" if ndim is None else " of %d dimensions" % ndim)
            raise _lib.OvnError("%s must be a contiguous %s tensor%s on %s%s"
                                % (what, dtype, size, self.device, " (or pinned host memory)" if pinned_ok else ""))
        return t

    def _poses64(self, poses) -> torch.Tensor:
        """Poses (a tensor or a host array) as a contiguous float64 tensor on the device."""
        if isinstance(poses, torch.Tensor):
            return poses.to(self.device, torch.float64).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float64))).to(self.device)

    def _image_outputs(self, n: int, h: int, w: int, table, want, channels: Optional[int] = None,
                       stacked_out: Optional[torch.Tensor] = None, min_channels: int = 0, out=None, what: str = ""):
        """The (n, h, w, ...) outputs of a call that makes images.  table: name -> (trailing shape, dtype) in the library's order.  An
        output is the caller's tensor when `out` holds its name, a fresh one when `want` names it, and absent otherwise.  channels:
        the stacked leg input's, None for a call that assembles none; it goes into `stacked_out` when given, which must have exactly
        `channels`, and is else allocated with max(channels, min_channels).  Returns (dict of the outputs present, stacked or None)."""
        bufs = {}
        for name, (tail, dt) in table.items():
            if out is not None and name in out:
                bufs[name] = self._check(out[name], "%sout[%r]" % (what, name), dt, (n, h, w) + tail)
            elif name in want:
                bufs[name] = torch.empty((n, h, w) + tail, dtype=dt, device=self.device)
        stk = None
        if channels is not None:
            if stacked_out is not None:
                stk = self._check(stacked_out, "stacked_out", _F32, (n, h, w, channels))
            else:
                stk = torch.empty((n, h, w, max(channels, min_channels)), dtype=_F32, device=self.device)
        return bufs, stk

    # -- weights ------------------------------------------------------------------------------------
    def load_weights(self, weights: Dict[str, np.ndarray], model_cfg: Optional[dict] = None) -> None:
        """Register leg + head weights given by Keras layer name (reference infer.py:117-120).  The optional model keys
        `correlationHead_normalize` (set_corr_normalization; a missing key leaves the mode as it is) and `deltaLayer_negateDiffs`
        (DeltaLayer(negateDiffs=True), generateNet.py:56-57: -|l - r|) are honoured here (weights.head_options).  c_conv1 is
        linear, so sum(-|d| w) + b = sum(|d| (-w)) + b with every product and partial sum equal up to sign: negated differences are
        registered as the negated c_conv1 kernel, exactly, in every head arithmetic."""
        cfg = model_cfg or {}
        norm, negate = W.head_options(cfg)
        try:     # the Dense kernel is sized by the width this leg produces (ovn_finalize refuses a geometry the heads cannot run)
            hf, fw, _ = W.leg_output_shape(self.in_h, self.in_w, W.leg_layers(self.in_c, cfg))
        except ValueError:
            hf, fw = 1, FEAT_W
        W.check_weights(weights, self.in_c, cfg, fw if hf == 1 else FEAT_W)
        self.conv1size = int(cfg.get("conv1NetworkHead_conv1size", 15))     # generateNet.py:88-89
        with self._dev():
            st = self._stream()
            for l in W.leg_layers(self.in_c, cfg):
                k = torch.from_numpy(np.ascontiguousarray(weights[l.name + "/kernel"], np.float32)).to(self.device)
                b = torch.from_numpy(np.ascontiguousarray(weights[l.name + "/bias"], np.float32)).to(self.device)
                self._call("ovn_add_leg_layer", l.name.encode(), _ptr(k), _ptr(b), l.kh, l.kw, l.cin, l.cout, l.sh, l.sw, st,
                           what="ovn_add_leg_layer(%s)" % l.name)
            fw = C.c_int(0)
            self._call("ovn_finalize", C.byref(fw))
            self.feat_w = fw.value
            self._leg_ready = True
            self._leg_cfg = {k: cfg[k] for k in ("strides_layer1", "additional_unsymmetric_layer3a") if k in cfg}
            if self.conv1size != 15:   # any other value: the library's general fp32 Delta path (no Delta cache)
                self._call("ovn_set_head_geometry", self.conv1size)
            names = ["c_conv1", "c_conv2", "c_conv3", "overlap_output"]
            ts = []
            for n in names:
                k = np.ascontiguousarray(weights[n + "/kernel"], np.float32)
                ts.append(torch.from_numpy(-k if (negate and n == "c_conv1") else k).to(self.device))
                ts.append(torch.from_numpy(np.ascontiguousarray(weights[n + "/bias"], np.float32)).to(self.device))
            self._call("ovn_set_head_weights", *[_ptr(t) for t in ts], st)
            self._head_ready = True
            self.negate_diffs = negate
            torch.cuda.synchronize(self.device)
        if "correlationHead_normalize" in cfg:
            self.set_corr_normalization(norm)

    # -- leg ----------------------------------------------------------------------------------------
    def leg(self, images: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images (n, H, W, C) float32 on this device -> feature volumes (n, feat_w, 128)."""
        self._require_leg()
        self._check(images, "leg input")
        if tuple(images.shape[1:]) != (self.in_h, self.in_w, self.in_c):
            raise _lib.OvnError("leg input shape %s, expected (n,%d,%d,%d)" % (tuple(images.shape), self.in_h, self.in_w, self.in_c))
        n = images.shape[0]
        if out is None:
            out = torch.empty((n, self.feat_w, FEAT_C), dtype=torch.float32, device=self.device)
        self._call("ovn_leg", _ptr(images), n, _ptr(out), self._stream())
        return out

    # -- heads --------------------------------------------------------------------------------------
    @property
    def _fw(self) -> int:
        """Width of this engine's feature volumes: the leg's output once the weights are loaded, 360 before."""
        return self.feat_w or FEAT_W

    @property
    def has_spectrum(self) -> bool:
        """The spectral correlation head (`spectrum`, `corr_head_spectral`, spec_l / spec_r of `heads`) runs 360-column volumes only."""
        return self._fw == FEAT_W

    def _require_head(self) -> None:
        if not self._head_ready:
            raise _lib.OvnError("head weights not loaded")

    def _require_spectrum(self) -> None:
        if not self.has_spectrum:
            raise _lib.OvnError("spectra exist for 360-column feature volumes only (this leg produces %d)" % self._fw)

    def _check_feats(self, t: torch.Tensor, what: str) -> int:
        """A stack of feature volumes; returns how many."""
        self._check(t, what)
        n, rest = divmod(t.numel(), self._fw * FEAT_C)
        if rest:
            raise _lib.OvnError("%s is not a stack of %dx128 feature volumes" % (what, self._fw))
        return n

    def _idx(self, idx, n: Optional[int], bound: Optional[int] = None, what: str = "pair index") -> Optional[torch.Tensor]:
        """Index list -> int32 device tensor.  Host lists / arrays are range-checked ON THE HOST before the upload (no device
        synchronisation).  A tensor that already lives on the device is TRUSTED (the caller built it; the kernels read
        feats[idx[p]] without a bound check, an out-of-range entry reads foreign memory) unless `self.check_device_indices` is set,
        which range-checks it on the device at the price of one synchronisation per call."""
        if idx is None:
            return None
        if isinstance(idx, torch.Tensor) and idx.device == self.device:
            if idx.dtype not in (torch.int32, torch.int64):
                raise IndexError("%s tensor must be int32 or int64, not %s" % (what, idx.dtype))
            if self.check_device_indices and bound is not None and idx.numel():
                lo, hi = int(idx.min()), int(idx.max())          # synchronises: opt-in (OvnEngine.check_device_indices)
                if lo < 0 or hi >= bound:
                    raise IndexError("%s out of range: [%d, %d] not within [0, %d)" % (what, lo, hi, bound))
            t = idx.to(torch.int32).contiguous()
        else:
            a = np.ascontiguousarray(idx.cpu().numpy() if isinstance(idx, torch.Tensor) else idx).reshape(-1)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                if not np.all(a == np.floor(a)):
                    raise IndexError("%s list holds non-integer values" % what)
            a = a.astype(np.int64)
            if bound is not None and a.size and (int(a.min()) < 0 or int(a.max()) >= bound):
                raise IndexError("%s out of range" % what)
            t = torch.from_numpy(a.astype(np.int32)).to(self.device)
        if n is not None and t.numel() != n:
            raise _lib.OvnError("index list has %d entries, expected %d" % (t.numel(), n))
        return t

    def _pairs(self, nl: int, nr: int, lidx, ridx, n: Optional[int]):
        """Shared argument checking of every head entry point: (lidx tensor | None, ridx tensor | None, n)."""
        li = self._idx(lidx, None, nl, "left pair index")
        if n is None:
            n = li.numel() if li is not None else nl
        n = int(n)
        if li is not None and li.numel() != n:
            raise _lib.OvnError("lidx has %d entries, expected %d" % (li.numel(), n))
        if li is None and n > nl:
            raise _lib.OvnError("n=%d pairs but only %d left feature volumes" % (n, nl))
        ri = self._idx(ridx, n, nr, "right pair index")
        if ri is None and n > 0 and nr < 1:
            raise _lib.OvnError("the right-hand side holds no feature volume")
        return li, ri, n

    def _heads_outputs(self, n: int, want_logit: bool, want_corr: bool):
        """(overlap (n) f32, yaw (n) i32, logit (n) f32 or None, corr (n, feat_w) f32 or None) for a call of both heads."""
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        return (f32(n), torch.empty(n, dtype=torch.int32, device=self.device), f32(n) if want_logit else None,
                f32(n, self._fw) if want_corr else None)

    @staticmethod
    def _heads_result(overlap, yaw, logit, corr) -> Dict[str, torch.Tensor]:
        out = {"overlap": overlap, "yaw": yaw}
        if logit is not None:
            out["logit"] = logit
        if corr is not None:
            out["corr"] = corr
        return out

    def heads(self, feats_l: torch.Tensor, feats_r: torch.Tensor, lidx=None, ridx=None, n: Optional[int] = None,
              want_logit: bool = False, want_corr: bool = False, spec_l: Optional[torch.Tensor] = None,
              spec_r: Optional[torch.Tensor] = None, dcache_l: Optional[torch.Tensor] = None):
        """Both heads on n pairs: pair p = (l = feats_l[lidx[p]], r = feats_r[ridx[p]]).
        lidx None -> p, ridx None -> 0 (1-vs-N: feats_r holds the single query).
        spec_l / spec_r: cached spectra (`spectrum`) -> the HBM-bound spectral yaw head; dcache_l: the left pool's Delta cache rows
        (`delta_cache`), used by 1-vs-N sweeps -- same results with or without it.
        Returns dict of device tensors: overlap (n) f32, yaw (n) i32 [, logit (n), corr (n, feat_w)].  At feat_w != 360 there are no
        spectra or Delta cache rows: spec_l / spec_r raise."""
        self._require_head()
        nl, nr = self._check_feats(feats_l, "feats_l"), self._check_feats(feats_r, "feats_r")
        li, ri, n = self._pairs(nl, nr, lidx, ridx, n)
        if spec_l is None and spec_r is None:
            overlap, yaw, logit, corr = self._heads_outputs(n, want_logit, want_corr)
            self._call("ovn_heads", _ptr(feats_l), _ptr(li), _ptr(feats_r), _ptr(ri), n, _ptr(overlap), _ptr(yaw), _ptr(logit), _ptr(corr),
                       self._stream())
            return self._heads_result(overlap, yaw, logit, corr)
        # cached spectra given: Delta head on the features, correlation head in its HBM-bound spectral form
        if spec_l is None or spec_r is None:
            raise _lib.OvnError("spec_l and spec_r must be given together")
        self._require_spectrum()
        self._check(spec_l, "spec_l", numel=nl * FEAT_C * self.SPEC_W)        # one 128x368 spectrum per feature volume
        self._check(spec_r, "spec_r", numel=nr * FEAT_C * self.SPEC_W)
        self._check(dcache_l, "dcache_l", numel=nl * self.DELTA_CACHE_ELEMS, optional=True)     # one row per left feature volume
        overlap, yaw, logit, corr = self._heads_outputs(n, want_logit, want_corr)
        self._call("ovn_heads_spectral", _ptr(feats_l), _ptr(spec_l), _ptr(dcache_l), _ptr(li), _ptr(feats_r), _ptr(spec_r), _ptr(ri), n,
                   _ptr(overlap), _ptr(yaw), _ptr(logit), _ptr(corr), self._stream())
        return self._heads_result(overlap, yaw, logit, corr)

    def heads_segments(self, feats_pool: torch.Tensor, feats_q: torch.Tensor, cand_idx, query_idx, seg_offsets,
                       spec_pool: Optional[torch.Tensor] = None, spec_q: Optional[torch.Tensor] = None,
                       dcache_pool: Optional[torch.Tensor] = None, want_logit: bool = False, want_corr: bool = False):
        """Both heads on a batch of B loop-closure queries in one call (`ovn_heads_segments`): segment b is the pairs
        [seg_offsets[b], seg_offsets[b + 1]), pair p = (left = feats_pool[cand_idx[p]], right = feats_q[query_idx[b]]) -- the 1-vs-N
        orientation of `Infer.infer_multiple`.  Pair p gets exactly the bits `heads` gives it when segment b runs alone in its 1-vs-N
        form (`heads(feats_pool, feats_q[q:q + 1], lidx=cand_idx[segment], spec_l=spec_pool, spec_r=spec_q[q:q + 1],
        dcache_l=dcache_pool)`).  seg_offsets / query_idx are host data (lists, arrays or tensors), checked here; cand_idx is
        range-checked on the host unless it is already a device tensor (see `_idx`).  spec_pool / spec_q: both or neither.
        The library stages the table through one pinned buffer: a segmented call (this one or `top_k_segments`) made while the
        previous one's table copy is still pending on its stream waits on the host for that copy; otherwise the call only enqueues.
        Returns dict of flat device tensors in pair order: overlap (n) f32, yaw (n) i32 [, logit (n), corr (n, feat_w)]."""
        self._require_head()
        npool, nq = self._check_feats(feats_pool, "feats_pool"), self._check_feats(feats_q, "feats_q")
        offs, q = segment_table(seg_offsets, query_idx, nq)
        n = int(offs[-1])
        ci = self._idx(cand_idx, n, npool, "candidate index")
        if (spec_pool is None) != (spec_q is None):
            raise _lib.OvnError("spec_pool and spec_q must be given together")
        if spec_pool is not None:
            self._require_spectrum()
            self._check(spec_pool, "spec_pool", numel=npool * FEAT_C * self.SPEC_W)     # one 128x368 spectrum per feature volume
            self._check(spec_q, "spec_q", numel=nq * FEAT_C * self.SPEC_W)
        self._check(dcache_pool, "dcache_pool", numel=npool * self.DELTA_CACHE_ELEMS, optional=True)     # one row per pool volume
        overlap, yaw, logit, corr = self._heads_outputs(n, want_logit, want_corr)
        self._call("ovn_heads_segments", _ptr(feats_pool), _ptr(spec_pool), _ptr(dcache_pool), _ptr(ci), _ptr(feats_q), _ptr(spec_q),
                   q.ctypes.data_as(C.POINTER(C.c_int32)), offs.ctypes.data_as(C.POINTER(C.c_int64)), len(q), n, _ptr(overlap),
                   _ptr(yaw), _ptr(logit), _ptr(corr), self._stream())
        return self._heads_result(overlap, yaw, logit, corr)

    def corr_head(self, feats_l: torch.Tensor, feats_r: torch.Tensor, lidx=None, ridx=None, n: Optional[int] = None,
                  want_corr: bool = False):
        li, ri, n = self._pairs(self._check_feats(feats_l, "feats_l"), self._check_feats(feats_r, "feats_r"), lidx, ridx, n)
        yaw = torch.empty(n, dtype=torch.int32, device=self.device)
        corr = torch.empty((n, self._fw), dtype=torch.float32, device=self.device) if want_corr else None
        self._call("ovn_corr_head", _ptr(feats_l), _ptr(li), _ptr(feats_r), _ptr(ri), n, _ptr(yaw), _ptr(corr), self._stream())
        return {"yaw": yaw, "corr": corr} if want_corr else {"yaw": yaw}

    # -- fitting the Delta head on frozen legs ---------------------------------------------------------
    HEAD_PARAMS = ("c_conv1/kernel", "c_conv1/bias", "c_conv2/kernel", "c_conv2/bias", "c_conv3/kernel", "c_conv3/bias",
                   "overlap_output/kernel", "overlap_output/bias")
    GRAD_PAIR_BLOCK = 4            # OVN_GRAD_PAIR_BLOCK of include/ovn_hip.h
    _LOSSES = {"sigmoid": 0, "mse": 1}

    def head_param_sizes(self) -> List[int]:
        """Elements of the eight head tensors (HEAD_PARAMS order) for this engine's conv1size and feature width."""
        sizes = (C.c_int64 * 8)()
        self._call("ovn_head_param_sizes", sizes)
        return [int(v) for v in sizes]

    def head_param_shapes(self) -> List[Tuple[int, ...]]:
        """Keras shapes of the eight head tensors (HEAD_PARAMS order)."""
        shapes = W.expected_shapes(self.in_c, {"conv1NetworkHead_conv1size": self.conv1size}, self._fw)
        return [tuple(shapes[k]) for k in self.HEAD_PARAMS]

    def set_head_weights(self, params: Sequence[torch.Tensor]) -> None:
        """Re-register the Delta head from eight float32 device tensors (HEAD_PARAMS order, Keras layouts, c_conv1 as the library
        holds it: negated under deltaLayer_negateDiffs).  Delta cache rows built under the old weights are stale afterwards."""
        if len(params) != 8:
            raise _lib.OvnError("set_head_weights takes the eight head tensors")
        ts = []
        for t, size in zip(params, self.head_param_sizes()):
            if t.device != self.device or t.dtype != torch.float32 or t.numel() != size:
                raise _lib.OvnError("head tensors must be float32 on %s with %s elements" % (self.device, self.head_param_sizes()))
            ts.append(t.contiguous())
        self._call("ovn_set_head_weights", *[_ptr(t) for t in ts], self._stream())
        self._head_ready = True

    def _grad_pairs(self, feats_l, feats_r, targets, lidx, ridx):
        """The arguments the two gradient calls share: (targets (n) f32 on the device, lidx, ridx, n >= 1)."""
        nl, nr = self._check_feats(feats_l, "feats_l"), self._check_feats(feats_r, "feats_r")
        if not isinstance(targets, torch.Tensor):
            targets = torch.from_numpy(np.ascontiguousarray(targets, np.float32))
        t = targets.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        li, ri, n = self._pairs(nl, nr, lidx, ridx, t.numel() if lidx is None else None)
        if n < 1 or t.numel() != n:
            raise _lib.OvnError("%d targets for %d pairs (at least one pair)" % (t.numel(), n))
        return t, li, ri, n

    def _head_grad_views(self, flat: torch.Tensor, sizes: List[int]) -> Dict[str, Dict[str, torch.Tensor]]:
        """layer name -> {'kernel', 'bias'}: the eight head gradients in their Keras shapes, views of `flat`."""
        grads: Dict[str, Dict[str, torch.Tensor]] = {}
        off = 0
        for name, size, shape in zip(self.HEAD_PARAMS, sizes, self.head_param_shapes()):
            layer, kind = name.split("/")
            grads.setdefault(layer, {})[kind] = flat[off:off + size].view(shape)
            off += size
        return grads

    def delta_head_grad(self, feats_l: torch.Tensor, feats_r: torch.Tensor, targets, lidx=None, ridx=None, loss: str = "sigmoid",
                        scale: float = 1.0, want_activations: bool = False):
        """Gradient of scale / n * sum_p loss(overlap_p, targets[p]) with respect to the eight head tensors as registered
        (`ovn_delta_head_grad`; pairs as in `heads`: lidx None -> p, ridx None -> 0).  loss: 'sigmoid' (the reference's
        my_sigmoid_loss) or 'mse'.  Returns dict: grads (layer name -> {'kernel', 'bias'} device tensors in Keras shapes, views of
        the one buffer 'flat'), loss (1,), overlap (n) [, o2 (n, G, G, 128), o3 (n, G - 2, G - 2, 256)]."""
        self._require_head()
        if loss not in self._LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(self._LOSSES), loss))
        if not np.isfinite(float(scale)):
            raise ValueError("scale must be finite")
        t, li, ri, n = self._grad_pairs(feats_l, feats_r, targets, lidx, ridx)
        sizes = self.head_param_sizes()
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        lossv = torch.empty(1, dtype=torch.float32, device=self.device)
        overlap = torch.empty(n, dtype=torch.float32, device=self.device)
        g = self._fw // self.conv1size
        o2 = torch.empty((n, g, g, 128), dtype=torch.float32, device=self.device) if want_activations else None
        o3 = torch.empty((n, g - 2, g - 2, 256), dtype=torch.float32, device=self.device) if want_activations else None
        self._call("ovn_delta_head_grad", _ptr(feats_l), _ptr(li), _ptr(feats_r), _ptr(ri), n, _ptr(t), self._LOSSES[loss], float(scale),
                   _ptr(flat), _ptr(lossv), _ptr(overlap), _ptr(o2), _ptr(o3), self._stream())
        out = {"grads": self._head_grad_views(flat, sizes), "flat": flat, "loss": lossv, "overlap": overlap}
        if want_activations:
            out["o2"], out["o3"] = o2, o3
        return out

    def heads_feature_grad(self, feats_l: torch.Tensor, feats_r: torch.Tensor, targets, yaw_bins=None, lidx=None, ridx=None,
                           loss: str = "sigmoid", overlap_scale: float = 5.0, yaw_scale: float = 1.0,
                           min_overlap_for_angle: float = 0.7, want_head_grads: bool = False, want_corr: bool = True):
        """Both heads' losses differentiated down to the feature volumes (`ovn_heads_feature_grad`; pairs as in `heads`).
        L_ov = overlap_scale / n sum_p loss(overlap_p, targets[p]) (the loss of `delta_head_grad`), L_yaw = yaw_scale / (n W) sum of
        the reference's weighted cross entropy of the W correlation logits against the one-hot of yaw_bins[p] (all zeros where
        targets[p] <= min_overlap_for_angle or the bin lies outside [0, W)).  yaw_bins None: no yaw part.
        Returns dict: dfeat_l, dfeat_r (n, W, 128): row p = the gradient reaching the volume pair p read (rows that address the same
        pool entry are NOT summed; `train.heads_loss` does that), loss_overlap, loss_yaw (0-dim views of 'loss' (2,)), overlap (n),
        corr (n, W): the correlation logits z, always un-normalised, whatever `set_corr_normalization` holds (want_corr=False leaves
        them out; a call without a yaw part then runs no correlation at all) [, grads, flat as `delta_head_grad` returns them for
        scale = overlap_scale]."""
        self._require_head()
        if loss not in self._LOSSES:
            raise ValueError("loss must be one of %s, got %r" % (sorted(self._LOSSES), loss))
        for name, v in (("overlap_scale", overlap_scale), ("yaw_scale", yaw_scale), ("min_overlap_for_angle", min_overlap_for_angle)):
            if not np.isfinite(float(v)):
                raise ValueError("%s must be finite" % name)
        t, li, ri, n = self._grad_pairs(feats_l, feats_r, targets, lidx, ridx)
        yb = None
        if yaw_bins is not None:
            if not isinstance(yaw_bins, torch.Tensor):
                yaw_bins = torch.from_numpy(np.ascontiguousarray(yaw_bins, np.int32))
            yb = yaw_bins.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if yb.numel() != n:
                raise _lib.OvnError("%d yaw bins for %d pairs" % (yb.numel(), n))
        dl = torch.empty((n, self._fw, FEAT_C), dtype=torch.float32, device=self.device)
        dr = torch.empty((n, self._fw, FEAT_C), dtype=torch.float32, device=self.device)
        lossv = torch.empty(2, dtype=torch.float32, device=self.device)
        overlap = torch.empty(n, dtype=torch.float32, device=self.device)
        corr = torch.empty((n, self._fw), dtype=torch.float32, device=self.device) if want_corr else None
        sizes = self.head_param_sizes()
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=self.device) if want_head_grads else None
        self._call("ovn_heads_feature_grad", _ptr(feats_l), _ptr(li), _ptr(feats_r), _ptr(ri), n, _ptr(t), _ptr(yb), self._LOSSES[loss],
                   float(overlap_scale), float(yaw_scale), float(min_overlap_for_angle), _ptr(dl), _ptr(dr), _ptr(flat), _ptr(lossv),
                   _ptr(overlap), _ptr(corr), self._stream())
        out = {"dfeat_l": dl, "dfeat_r": dr, "loss": lossv, "loss_overlap": lossv[0], "loss_yaw": lossv[1], "overlap": overlap}
        if want_corr:
            out["corr"] = corr
        if want_head_grads:
            out["grads"], out["flat"] = self._head_grad_views(flat, sizes), flat
        return out

    # -- training the legs ---------------------------------------------------------------------------------
    LEG_GRAD_SCAN_BLOCK = 4        # OVN_LEG_GRAD_SCAN_BLOCK of include/ovn_hip.h

    def _require_leg(self) -> None:
        if not self._leg_ready:
            raise _lib.OvnError("leg weights not loaded")

    def _leg_specs(self) -> List[Tuple[str, Tuple[int, ...]]]:
        """(layer name, Keras kernel shape) of the registered leg layers, in network order."""
        return [(l.name, (l.kh, l.kw, l.cin, l.cout)) for l in W.leg_layers(self.in_c, self._leg_cfg)]

    def leg_param_names(self) -> List[str]:
        """Keras names of the 2 x layers leg tensors in the library's order: s_conv1/kernel, s_conv1/bias, s_conv2/kernel, ..."""
        return [n + "/" + kind for n, _ in self._leg_specs() for kind in ("kernel", "bias")]

    def leg_param_shapes(self) -> List[Tuple[int, ...]]:
        """Keras shapes of the leg tensors (leg_param_names order), checked against `ovn_leg_param_sizes`."""
        self._require_leg()
        shapes = [s for _, k in self._leg_specs() for s in (k, (k[3],))]
        nl = C.c_int(0)
        self._call("ovn_leg_layer_count", C.byref(nl))
        sizes = (C.c_int64 * (2 * nl.value))()
        self._call("ovn_leg_param_sizes", sizes)
        if [int(v) for v in sizes] != [int(np.prod(s)) for s in shapes]:
            raise _lib.OvnError("the library holds leg tensors of %s elements, the layer table says %s"
                                % ([int(v) for v in sizes], shapes))
        return shapes

    def leg_activation_shapes(self) -> List[Tuple[int, int, int]]:
        """(oh, ow, cout) of every leg layer's output for this engine's input geometry, checked against `ovn_leg_activation_sizes`."""
        self._require_leg()
        h, w, shapes = self.in_h, self.in_w, []
        for l in W.leg_layers(self.in_c, self._leg_cfg):
            h, w = (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1
            shapes.append((h, w, l.cout))
        sizes = (C.c_int64 * len(shapes))()
        self._call("ovn_leg_activation_sizes", sizes)
        if [int(v) for v in sizes] != [a * b * c for a, b, c in shapes]:
            raise _lib.OvnError("the library's leg activations %s do not match the layer table %s" % ([int(v) for v in sizes], shapes))
        return shapes

    def _check_images(self, images: torch.Tensor) -> int:
        self._check(images, "leg input")
        if images.dim() != 4 or tuple(images.shape[1:]) != (self.in_h, self.in_w, self.in_c) or images.shape[0] < 1:
            raise _lib.OvnError("leg input shape %s, expected (n >= 1,%d,%d,%d)" % (tuple(images.shape), self.in_h, self.in_w, self.in_c))
        return int(images.shape[0])

    def leg_forward_train(self, images: torch.Tensor) -> List[torch.Tensor]:
        """images (n, H, W, C) -> the list of every leg layer's post-ReLU output (n, oh, ow, cout), in exact fp32 whatever
        `set_leg_precision` says (`ovn_leg_forward_train`).  The tensors are views of ONE layer-major buffer, which `leg_backward`
        takes back; the last one, viewed (n, feat_w, 128), is the feature volumes."""
        self._require_leg()
        n = self._check_images(images)
        shapes = self.leg_activation_shapes()
        flat = torch.empty(n * sum(a * b * c for a, b, c in shapes), dtype=torch.float32, device=self.device)
        self._call("ovn_leg_forward_train", _ptr(images), n, _ptr(flat), self._stream())
        acts, off = [], 0
        for a, b, c in shapes:
            acts.append(flat[off:off + n * a * b * c].view(n, a, b, c))
            off += n * a * b * c
        return acts

    def leg_backward(self, images: torch.Tensor, acts: Sequence[torch.Tensor], dfeat: torch.Tensor, slice_scans: int = 0):
        """Gradients of the 2 x layers leg tensors, summed over the n scans, from dfeat (n, feat_w, 128) = dL/d(feature volume of
        scan i) (`ovn_leg_backward`).  acts: what `leg_forward_train` returned for `images`.  Returns dict: Keras name
        ('s_conv1/kernel', ...) -> device tensor in its Keras shape (views of the one buffer 'flat')."""
        self._require_leg()
        n = self._check_images(images)
        shapes = self.leg_activation_shapes()
        if len(acts) != len(shapes):
            raise _lib.OvnError("leg_backward takes the %d activations of leg_forward_train" % len(shapes))
        base = acts[0].data_ptr()
        off = 0
        for i, (t, (a, b, c)) in enumerate(zip(acts, shapes)):
            self._check(t, "leg_backward: acts[%d]" % i, shape=(n, a, b, c))
            if t.data_ptr() != base + 4 * off:
                raise _lib.OvnError("leg_backward: acts must be the list leg_forward_train returned for these %d scans" % n)
            off += n * a * b * c
        self._check(dfeat, "dfeat", numel=n * self.feat_w * FEAT_C)       # n feature volumes
        if int(slice_scans) < 0:
            raise ValueError("slice_scans must be >= 0")
        pshapes = self.leg_param_shapes()
        flat = torch.empty(sum(int(np.prod(s)) for s in pshapes), dtype=torch.float32, device=self.device)
        self._call("ovn_leg_backward", _ptr(images), C.c_void_p(base), n, _ptr(dfeat), _ptr(flat), int(slice_scans), self._stream())
        out: Dict[str, torch.Tensor] = {}
        off = 0
        for name, shape in zip(self.leg_param_names(), pshapes):
            size = int(np.prod(shape))
            out[name] = flat[off:off + size].view(shape)
            off += size
        out["flat"] = flat
        return out

    def set_leg_weights(self, params) -> None:
        """Replace leg weights in place (`ovn_set_leg_layer_weights`).  params: dict Keras name -> float32 device tensor (both tensors
        of every layer it names), or the full list in `leg_param_names` order.  Feature volumes, spectra and Delta cache rows
        computed by the old legs are stale afterwards."""
        self._require_leg()
        names, shapes = self.leg_param_names(), self.leg_param_shapes()
        if not isinstance(params, dict):
            if len(params) != len(names):
                raise _lib.OvnError("set_leg_weights takes the %d leg tensors" % len(names))
            params = dict(zip(names, params))
        for li, (layer, _) in enumerate(self._leg_specs()):
            k, b = params.get(layer + "/kernel"), params.get(layer + "/bias")
            if k is None and b is None:
                continue
            if k is None or b is None:
                raise _lib.OvnError("set_leg_weights: layer %s needs its kernel and its bias" % layer)
            for t, shape in ((k, shapes[2 * li]), (b, shapes[2 * li + 1])):
                if t.device != self.device or t.dtype != torch.float32 or t.numel() != int(np.prod(shape)):
                    raise _lib.OvnError("set_leg_weights: %s tensors must be float32 on %s with shapes %s, %s"
                                        % (layer, self.device, shapes[2 * li], shapes[2 * li + 1]))
            k, b = k.contiguous(), b.contiguous()
            self._call("ovn_set_leg_layer_weights", li, _ptr(k), _ptr(b), self._stream(), what="ovn_set_leg_layer_weights(%s)" % layer)

    # -- data-parallel training ------------------------------------------------------------------------------
    GRAD_REDUCE_MAX_WORLD = 64     # OVN_GRAD_REDUCE_MAX_WORLD of include/ovn_hip.h

    def grad_reduce_adagrad(self, grads: torch.Tensor, rank_weights, params: Optional[torch.Tensor] = None,
                            accum: Optional[torch.Tensor] = None, lr: float = 0.0, eps: float = 1e-7, want_grad: bool = False,
                            count: Optional[int] = None):
        """The ranks' gradients reduced and Adagrad applied in one kernel (`ovn_grad_reduce_adagrad`).  grads (world, stride) float32,
        stride a multiple of 4: row r is rank r's flat gradient; rank_weights: world host numbers n_r / n (a row with weight 0 is not
        read).  params / accum: flat float32 tensors of count <= stride elements, updated IN PLACE with
        g = float32(sum_r w_r G[r] in fp64, rank order); a += g g; p -= lr g / (sqrt(a) + eps); both None: reduce only (the first
        `count` elements of the rows, default all).  Returns the reduced gradient (count) when want_grad or when only reducing, else None."""
        self._check(grads, "grads (world, stride)", ndim=2)
        world, stride = int(grads.shape[0]), int(grads.shape[1])
        w = np.ascontiguousarray(np.asarray(rank_weights, np.float64).reshape(-1))
        if len(w) != world or not 1 <= world <= self.GRAD_REDUCE_MAX_WORLD:
            raise _lib.OvnError("%d rank weights for %d gradient rows (1 .. %d ranks)" % (len(w), world, self.GRAD_REDUCE_MAX_WORLD))
        if (params is None) != (accum is None):
            raise _lib.OvnError("params and accum are given together or not at all")
        if params is None:
            count = stride if count is None else int(count)
            if not 1 <= count <= stride:
                raise _lib.OvnError("count %d for gradient rows of %d" % (count, stride))
        else:
            self._check(params, "params", ndim=1)
            self._check(accum, "accum", ndim=1)
            count = int(params.numel())
            if accum.numel() != count or not 1 <= count <= stride:
                raise _lib.OvnError("params %d and accum %d elements for gradient rows of %d" % (count, accum.numel(), stride))
        out = torch.empty(count, dtype=torch.float32, device=self.device) if (want_grad or params is None) else None
        self._call("ovn_grad_reduce_adagrad", _ptr(grads), world, stride, w.ctypes.data_as(C.POINTER(C.c_double)), count, _ptr(params),
                   _ptr(accum), float(lr), float(eps), _ptr(out), self._stream())
        return out

    def debug_conv(self, layer: int, x: torch.Tensor) -> torch.Tensor:
        """Leg layer `layer` alone on x (nb, h, w, cin) in the current leg precision (`ovn_debug_conv`)."""
        self._require_leg()
        l = W.leg_layers(self.in_c, self._leg_cfg)[layer]
        nb, h, w, _ = x.shape
        out = torch.empty((nb, (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1, l.cout), dtype=torch.float32, device=self.device)
        self._call("ovn_debug_conv", int(layer), _ptr(x.contiguous()), nb, h, w, _ptr(out), self._stream())
        return out

    def debug_conv_grad(self, layer: int, x: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, want=("din", "dkernel", "dbias")):
        """The gradients of leg layer `layer` alone (`ovn_debug_conv_grad`): x (nb, h, w, cin) its input, out (nb, oh, ow, cout) its
        post-ReLU output (the mask), dout = dL/d(out).  Returns dict of the requested 'din' (nb, h, w, cin), 'dkernel' (Keras
        shape), 'dbias' (cout).  din of a layer whose cin is not a multiple of 16 comes from a plain fp64 kernel."""
        self._require_leg()
        specs = W.leg_layers(self.in_c, self._leg_cfg)
        if not 0 <= int(layer) < len(specs):
            raise IndexError("no leg layer %r" % (layer,))
        l = specs[int(layer)]
        for t, name in ((x, "x"), (out, "out"), (dout, "dout")):
            self._check(t, "debug_conv_grad: " + name)
        if x.dim() != 4 or x.shape[3] != l.cin or x.shape[0] < 1 or x.shape[1] < l.kh or x.shape[2] < l.kw:
            raise _lib.OvnError("debug_conv_grad: input shape %s for layer %s" % (tuple(x.shape), l.name))
        nb, h, w, _ = (int(v) for v in x.shape)
        oshape = (nb, (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1, l.cout)
        if tuple(out.shape) != oshape or tuple(dout.shape) != oshape:
            raise _lib.OvnError("debug_conv_grad: out / dout must be %s" % (oshape,))
        r = {}
        if "din" in want:
            r["din"] = torch.empty_like(x)
        if "dkernel" in want:
            r["dkernel"] = torch.empty((l.kh, l.kw, l.cin, l.cout), dtype=torch.float32, device=self.device)
        if "dbias" in want:
            r["dbias"] = torch.empty(l.cout, dtype=torch.float32, device=self.device)
        self._call("ovn_debug_conv_grad", int(layer), _ptr(x), _ptr(out), _ptr(dout), nb, h, w, _ptr(r.get("din")), _ptr(r.get("dkernel")),
                   _ptr(r.get("dbias")), self._stream())
        return r

    SPEC_W = 368
    DELTA_CACHE_ELEMS = 49216     # floats per Delta cache row (include/ovn_hip.h: OVN_DELTA_CACHE_ELEMS)

    @property
    def has_delta_cache(self) -> bool:
        # the bf16x3 head mode reads no Delta cache rows, so none are built for it; nor are they at a feature width other than 360
        return self.conv1size == 15 and self.head_precision != "bf16x3" and self._fw == FEAT_W

    def delta_cache(self, feats: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feature volumes (n,360,128) -> Delta cache rows (n, 49216): the candidate-side half of the Delta head's preparation
        (packed words, TT + b2, value range), cached next to the volume like its spectrum."""
        self._require_head()
        if not self.has_delta_cache:
            raise _lib.OvnError("the Delta cache exists for conv1NetworkHead_conv1size=15 and 360-column feature volumes only")
        n = self._check_feats(feats, "feats")
        if out is None:
            out = torch.empty((n, self.DELTA_CACHE_ELEMS), dtype=torch.float32, device=self.device)
        self._call("ovn_delta_cache", _ptr(feats), n, _ptr(out), self._stream())
        return out

    def spectrum(self, feats: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """feature volumes (n,360,128) -> cached spectra (n,128,368) for the spectral correlation head (360 columns only)."""
        self._require_spectrum()
        n = self._check_feats(feats, "feats")
        if out is None:
            out = torch.empty((n, FEAT_C, self.SPEC_W), dtype=torch.float32, device=self.device)
        self._call("ovn_spectrum", _ptr(feats), n, _ptr(out), self._stream())
        return out

    def corr_head_spectral(self, spec_l: torch.Tensor, spec_r: torch.Tensor, lidx=None, ridx=None,
                           n: Optional[int] = None, want_corr: bool = False):
        """Correlation head on cached spectra: dict(yaw (n) i32 [, corr (n,360)]); 360-column feature volumes only."""
        self._require_spectrum()
        for t, what in ((spec_l, "spec_l"), (spec_r, "spec_r")):
            self._check(t, what)
            if t.numel() % (FEAT_C * self.SPEC_W) != 0:
                raise _lib.OvnError("%s is not a stack of 128x368 spectra" % what)
        li, ri, n = self._pairs(spec_l.numel() // (FEAT_C * self.SPEC_W), spec_r.numel() // (FEAT_C * self.SPEC_W), lidx, ridx, n)
        yaw = torch.empty(n, dtype=torch.int32, device=self.device)
        corr = torch.empty((n, FEAT_W), dtype=torch.float32, device=self.device) if want_corr else None
        self._call("ovn_corr_head_spectral", _ptr(spec_l), _ptr(li), _ptr(spec_r), _ptr(ri), n, _ptr(yaw), _ptr(corr), self._stream())
        return {"yaw": yaw, "corr": corr} if want_corr else {"yaw": yaw}

    # -- ground-truth labels -------------------------------------------------------------------------
    def gt_range_images(self, points: torch.Tensor, offsets: torch.Tensor, max_points: int,
                        ref_poses: Optional[torch.Tensor] = None, inv_cur_pose: Optional[torch.Tensor] = None,
                        proj_h: int = 64, proj_w: int = 900, fov_up: float = 3.0, fov_down: float = -25.0,
                        max_range: float = 50.0) -> torch.Tensor:
        """Float64 range projection of scans moved by inv_cur_pose . ref_poses[s] (com_overlap_yaw.py:37-40):
        (n, H, W) f32 device tensor, -1 = empty.  points (total,4) f32, offsets (n+1) i64, poses float64 device tensors."""
        n = int(offsets.numel()) - 1
        self._check(points, "points")
        self._check(offsets, "offsets", torch.int64)
        self._check(ref_poses, "ref_poses (%d 4x4 matrices)" % n, torch.float64, numel=16 * n, optional=True)
        self._check(inv_cur_pose, "inv_cur_pose (one 4x4 matrix)", torch.float64, numel=16, optional=True)
        out = torch.empty((n, proj_h, proj_w), dtype=torch.float32, device=self.device)
        self._call("ovn_gt_range_images", _ptr(points), _ptr(offsets), n, int(max_points), _ptr(ref_poses), _ptr(inv_cur_pose), proj_h,
                   proj_w, float(fov_up), float(fov_down), float(max_range), _ptr(out), self._stream())
        return out

    def gt_overlap_counts(self, ref_ranges: torch.Tensor, cur_range: torch.Tensor) -> torch.Tensor:
        """(n+1) int32: per reference scan the pixels with |ref - cur| < 1 (ref > 0); last entry = #{cur > 0}."""
        n, h, w = ref_ranges.shape
        self._check(ref_ranges, "ref_ranges")
        self._check(cur_range, "cur_range")
        if tuple(cur_range.shape[-2:]) != (h, w) or cur_range.numel() != h * w:
            raise _lib.OvnError("cur_range must be one %dx%d image" % (h, w))
        counts = torch.empty(n + 1, dtype=torch.int32, device=self.device)
        self._call("ovn_gt_overlap_counts", _ptr(ref_ranges), _ptr(cur_range), n, h, w, _ptr(counts), self._stream())
        return counts

    def gt_pair_counts(self, points: torch.Tensor, offsets: torch.Tensor, poses: torch.Tensor, inv_poses: torch.Tensor,
                       cur_ranges: torch.Tensor, frame_idx: Optional[torch.Tensor] = None,
                       ref_idx: Optional[torch.Tensor] = None, fov_up: float = 3.0, fov_down: float = -25.0,
                       max_range: float = 50.0) -> torch.Tensor:
        """(F, R) int32 device tensor: for frame frame_idx[f] and scan ref_idx[r] the integer `gt_overlap_counts` gives for that
        pair, from one kernel without the pair's range image.  points (total,4) f32 and offsets (n+1) i64 of all n scans, poses
        and inv_poses (n,4,4) f64, cur_ranges (n,H,W) f32 = `gt_range_images` without poses (rows of scans that are no frame are
        never read), frame_idx / ref_idx int32 device lists or None = all scans in order."""
        n = int(offsets.numel()) - 1
        self._check(points, "points")
        self._check(offsets, "offsets", torch.int64)
        self._check(poses, "poses (%d 4x4 matrices)" % n, torch.float64, numel=16 * n)
        self._check(inv_poses, "inv_poses (%d 4x4 matrices)" % n, torch.float64, numel=16 * n)
        self._check(cur_ranges, "cur_ranges", ndim=3)
        self._check(frame_idx, "frame_idx", torch.int32, optional=True)
        self._check(ref_idx, "ref_idx", torch.int32, optional=True)
        if cur_ranges.shape[0] != n:
            raise _lib.OvnError("cur_ranges must be (%d, H, W), one own range image per scan" % n)
        h, w = int(cur_ranges.shape[1]), int(cur_ranges.shape[2])
        nf = n if frame_idx is None else int(frame_idx.numel())
        nr = n if ref_idx is None else int(ref_idx.numel())
        counts = torch.empty((nf, nr), dtype=torch.int32, device=self.device)
        self._call("ovn_gt_pair_counts", _ptr(points), _ptr(offsets), n, _ptr(poses), _ptr(inv_poses), _ptr(cur_ranges), _ptr(frame_idx),
                   nf, _ptr(ref_idx), nr, h, w, float(fov_up), float(fov_down), float(max_range), _ptr(counts), self._stream())
        return counts

    # -- loop-closure decision -----------------------------------------------------------------------
    def _check_scores(self, n: int, overlap: torch.Tensor, yaw: Optional[torch.Tensor], ids: Optional[torch.Tensor]) -> None:
        """The scores of a sweep as the decision calls take them: overlap f32, yaw and ids int32 or None, n elements each."""
        self._check(overlap, "overlap", torch.float32, numel=n)
        self._check(yaw, "yaw", torch.int32, numel=n, optional=True)
        self._check(ids, "ids", torch.int32, numel=n, optional=True)

    def best_match(self, overlap: torch.Tensor, yaw: Optional[torch.Tensor] = None, threshold: float = 0.3,
                   ids: Optional[torch.Tensor] = None, index_offset: int = 0, host: bool = False) -> torch.Tensor:
        """On-device `argmax overlap, > threshold` of demo3 (demo3_lcd.py:117-120).  Returns a 4 x int32 device
        record {candidate id, float bits of overlap, yaw, found}; decode with `decode_match`.  host=True: the kernel writes the
        record straight into pinned host memory (device-visible at the same address) and the call waits for the stream -- the
        caller reads the decision without a device-to-host copy (one blit kernel and its hand-off less per query); the record comes back
        as a NumPy int32 array."""
        n = int(overlap.numel())
        self._check_scores(n, overlap, yaw, ids)
        if host:
            if getattr(self, "_match_host", None) is None:
                self._match_host = torch.empty(4, dtype=torch.int32).pin_memory()
                self._match_host_np = self._match_host.numpy()          # the same memory
            out, view = self._match_host, self._match_host_np
            view[3] = _MATCH_PENDING                                      # the kernel's one 16-byte store replaces it (0 or 1)
        else:
            out = torch.empty(4, dtype=torch.int32, device=self.device)
        self._call("ovn_best_match", _ptr(overlap), _ptr(yaw), _ptr(ids), n, float(threshold), int(index_offset), _ptr(out), self._stream())
        if host:
            # poll the record instead of waiting for the stream: the wake-up of a stream wait costs more than the kernel
            spins = 0
            while view[3] == _MATCH_PENDING:
                spins += 1
                if spins > 200000:                                    # (~20 ms) something is wrong: let the stream say what
                    torch.cuda.current_stream(self.device).synchronize()
                    if view[3] == _MATCH_PENDING:
                        raise _lib.OvnError("best_match(host=True): the decision record never arrived")
            return view.copy()            # (a NumPy record: `decode_match` takes it as it is)
        return out

    def top_k(self, overlap: torch.Tensor, yaw: Optional[torch.Tensor] = None, k: int = 5, threshold: float = 0.3,
              ids: Optional[torch.Tensor] = None, index_offset: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The k best candidates of a 1-vs-N sweep, ranked on the device (`ovn_top_k`): a (k, 4) int32 device tensor of
        best-match records, best first -- overlap descending, equal overlaps by position ascending, -0 == +0, NaN never selected,
        {-1, 0, 0, 0} past the last non-NaN score.  k = 1 gives `best_match`'s record bit for bit.  Decode with `decode_top_k`.
        `out` (optional): a contiguous int32 device tensor of k x 4 elements, 16-byte aligned (the library checks)."""
        n = int(overlap.numel())
        self._check_scores(n, overlap, yaw, ids)
        k = int(k)
        if out is None:
            out = torch.empty((max(k, 0), 4), dtype=torch.int32, device=self.device)
        else:
            self._check(out, "out", torch.int32, numel=4 * k)
        self._call("ovn_top_k", _ptr(overlap), _ptr(yaw), _ptr(ids), n, k, float(threshold), int(index_offset), _ptr(out), self._stream())
        return out

    def top_k_segments(self, overlap: torch.Tensor, seg_offsets, yaw: Optional[torch.Tensor] = None, k: int = 5,
                       threshold: float = 0.3, ids: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`top_k` of every segment of a `heads_segments` batch in one launch (`ovn_top_k_segments`): a (B, k, 4) int32 device
        tensor; segment b's k records are bit for bit `top_k(overlap[o0:o1], yaw[o0:o1], k, threshold, ids=ids[o0:o1])` (ids None:
        the position inside the segment); an empty segment gives k records {-1, 0, 0, 0}.  seg_offsets: host data, checked here.
        Shares `heads_segments`' pinned staging buffer, and with it the host wait for a table copy that is still pending."""
        offs, _ = segment_table(seg_offsets, None, None)
        k = check_top_k(k)
        n, B = int(offs[-1]), len(offs) - 1
        self._check_scores(n, overlap, yaw, ids)
        if out is None:
            out = torch.empty((B, k, 4), dtype=torch.int32, device=self.device)
        else:
            self._check(out, "out", torch.int32, numel=4 * k * B)
        self._call("ovn_top_k_segments", _ptr(overlap), _ptr(yaw), _ptr(ids), offs.ctypes.data_as(C.POINTER(C.c_int64)), B, k,
                   float(threshold), _ptr(out), self._stream())
        return out

    # -- preprocessing ------------------------------------------------------------------------------
    def project(self, points: torch.Tensor, offsets: torch.Tensor, max_points: int, proj_h: int = 64,
                proj_w: int = 900, fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0,
                want: Sequence[str] = ("range", "normal", "intensity"), stacked_flags: Optional[Tuple[bool, ...]] = None,
                stacked_out: Optional[torch.Tensor] = None, probs: Optional[torch.Tensor] = None, n_classes: int = 20,
                n_points: Optional[int] = None):
        """Batch spherical projection.  points: (total,4) f32 device tensor of concatenated scans,
        offsets: (n_scans+1) int64 device tensor (absolute positions in `points`: a slice of a longer offsets tensor projects
        that range of scans).  `want` selects outputs among range, vertex, intensity, idx, normal;
        stacked_flags=(use_depth,use_normals,use_intensity) additionally assembles the (n,H,W,C) leg input (into `stacked_out`
        when given).  Returns a dict of device tensors.
        probs: (offsets[-1], n_classes) f32 device tensor of per-point class probabilities (the semantic model's input,
        gen_semantic_data.py:33-46) -- routes the call to ovn_project_semantic: `want` may then also name "semantic"
        (n,H,W,n_classes: the probabilities of each pixel's point under max_range = inf, -1 elsewhere) and "sem_idx" (that
        point's proj_idx, which indexes the unfiltered rows as in the reference), stacked_flags is
        (use_depth, use_normals, use_semantic, use_intensity) in the reference's channel order, and every other output is bit
        for bit the one of the call without probs.  n_points: offsets[-1] when the caller knows it (else read from the device)."""
        self._check(points, "points")
        if offsets.device != self.device or offsets.dtype != torch.int64:
            raise _lib.OvnError("offsets must be an int64 tensor on %s" % self.device)
        semantic = probs is not None
        table = _PROJECT_OUTPUTS
        if semantic:
            n_classes = int(n_classes)
            if not 1 <= n_classes <= SEMANTIC_CLASSES_MAX:
                raise _lib.OvnError("n_classes must be in 1..%d, got %d" % (SEMANTIC_CLASSES_MAX, n_classes))
            total = int(offsets[-1].item()) if n_points is None else int(n_points)
            self._check(probs, "probs (one row per point)", shape=(total, n_classes))
            if probs.numel() == 0:      # no points at all: nothing is read, but the library wants a buffer for a probability output
                probs = torch.empty((1, n_classes), dtype=torch.float32, device=self.device)
            if stacked_flags is not None and len(stacked_flags) != 4:
                raise _lib.OvnError("with probs, stacked_flags is (use_depth, use_normals, use_semantic, use_intensity)")
            table = dict(_PROJECT_OUTPUTS, semantic=((n_classes,), _F32), sem_idx=((), _I32))
        n = offsets.numel() - 1
        ud = un = us = ui = 0
        c = None
        if stacked_flags is not None:
            if semantic:
                ud, un, us, ui = (int(bool(v)) for v in stacked_flags)
            else:
                ud, un, ui = (int(bool(v)) for v in stacked_flags)
            c = ud + 3 * un + ui + (n_classes if us else 0)
        out, stk = self._image_outputs(n, proj_h, proj_w, table, want, c, stacked_out)
        scans = (_ptr(points), _ptr(offsets), n, int(max_points), proj_h, proj_w, float(fov_up), float(fov_down), float(max_range))
        images = [_ptr(out.get(k)) for k in table]
        if semantic:
            self._call("ovn_project_semantic", *scans, _ptr(probs), n_classes, *images, _ptr(stk), ud, un, us, ui, self._stream())
        else:
            self._call("ovn_project", *scans, *images, _ptr(stk), ud, un, ui, self._stream())
        if stk is not None:
            out["stacked"] = stk
        return out

    def normals(self, rng: torch.Tensor, vtx: torch.Tensor) -> torch.Tensor:
        """range (n,H,W) + vertex (n,H,W,4) device tensors -> normal map (n,H,W,3)."""
        self._check(rng, "normals(): range")
        self._check(vtx, "normals(): vertex")
        n, h, w = rng.shape
        if tuple(vtx.shape) != (n, h, w, 4):
            raise _lib.OvnError("normals(): vertex shape %s does not match range %s" % (tuple(vtx.shape), tuple(rng.shape)))
        out = torch.empty((n, h, w, 3), dtype=torch.float32, device=self.device)
        self._call("ovn_normals", _ptr(rng), _ptr(vtx), n, h, w, _ptr(out), self._stream())
        return out

    def render_scans(self, mesh, poses, proj_h: int = 64, proj_w: int = 900, fov_up: float = 3.0, fov_down: float = -25.0,
                     max_range: float = 50.0, want: Sequence[str] = ("range", "normal"),
                     stacked_flags: Optional[Tuple[bool, ...]] = None, stacked_out: Optional[torch.Tensor] = None,
                     exhaustive: bool = False):
        """Virtual scans of a `mesh.TriangleMesh` from `poses` ((n,4,4) float64 sensor-to-world, host array or device tensor), one ray
        per pixel (ovn_render_scans).  `want` selects outputs among range, tri_id, vertex, normal; stacked_flags = (use_depth,
        use_normals) additionally assembles the (n,H,W,C) leg input (into `stacked_out` when given); a third (intensity) or fourth
        (class probabilities) flag that is set is refused by the library: a rendered scan has neither.  exhaustive=True walks every
        triangle with every ray (the validation route) instead of the mesh's hierarchy.  Returns a dict of device tensors."""
        bad = [k for k in want if k not in _RENDER_OUTPUTS]
        if bad:
            raise _lib.OvnError("render_scans: no output %s (a rendered scan has range, tri_id, vertex, normal)" % bad)
        p = self._poses64(poses)
        if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
            raise _lib.OvnError("render_scans: poses must be (n,4,4), got %s" % (tuple(p.shape),))
        n = p.shape[0]
        proj_h, proj_w = int(proj_h), int(proj_w)
        tabs = self._direction_tables(proj_h, proj_w, fov_up, fov_down)
        md = mesh.device(self, with_bvh=not exhaustive)
        nodes, order, leaves = (None, None, 0) if exhaustive else (md["nodes"], md["order"], md["leaves"])
        flags = [0, 0, 0, 0]
        c = None
        if stacked_flags is not None:
            if not 1 <= len(stacked_flags) <= 4:
                raise _lib.OvnError("render_scans: stacked_flags is (use_depth, use_normals[, use_intensity[, use_semantic]])")
            flags[:len(stacked_flags)] = [int(bool(v)) for v in stacked_flags]
            c = flags[0] + 3 * flags[1]
        out, stk = self._image_outputs(n, proj_h, proj_w, _RENDER_OUTPUTS, want, c, stacked_out, min_channels=1)
        self._call("ovn_render_scans", _ptr(md["vertices"]), mesh.n_vertices, _ptr(md["triangles"]), mesh.n_triangles, _ptr(nodes),
                   _ptr(order), int(leaves), _ptr(p), n, proj_h, proj_w, _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), _ptr(tabs[3]),
                   float(max_range), *[_ptr(out.get(k)) for k in _RENDER_OUTPUTS], _ptr(stk), *flags, self._stream())
        if stk is not None:
            out["stacked"] = stk
        return out

    def _tsdf_volume_args(self, what: str, tsdf: torch.Tensor, weight: torch.Tensor, origin):
        self._check(tsdf, "%s: tsdf (nz,ny,nx)" % what, ndim=3)
        self._check(weight, "%s: weight (nz,ny,nx)" % what, ndim=3)
        if tuple(weight.shape) != tuple(tsdf.shape):
            raise _lib.OvnError("%s: weight %s does not match tsdf %s" % (what, tuple(weight.shape), tuple(tsdf.shape)))
        org = np.asarray(origin, np.float64).reshape(-1)
        if org.shape[0] != 3:
            raise _lib.OvnError("%s: origin must hold 3 numbers, got %d" % (what, org.shape[0]))
        nz, ny, nx = (int(v) for v in tsdf.shape)
        return nx, ny, nz, (C.c_double * 3)(*org)

    @staticmethod
    def _int3(what: str, name: str, v):
        """3 int32 on the host for the library: a window's base or a box of cells."""
        a = np.asarray(v).reshape(-1)
        if a.shape[0] != 3 or not np.issubdtype(a.dtype, np.integer):
            raise _lib.OvnError("%s: %s must hold 3 integers, got %r" % (what, name, v))
        if np.any(np.abs(a.astype(np.int64)) >= 2 ** 31):
            raise _lib.OvnError("%s: %s %s does not fit int32" % (what, name, a.tolist()))
        return (C.c_int32 * 3)(*(int(x) for x in a))

    def tsdf_integrate(self, tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel: float, trunc: float, max_weight: float,
                       range_images: torch.Tensor, poses, fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0,
                       base=None) -> None:
        """Fuses `range_images` ((n,H,W) float32 device tensor, -1 = empty) taken at `poses` ((n,4,4) float64 sensor-to-world, host
        array or device tensor) into the volume tsdf / weight ((nz,ny,nx) float32 device tensors, updated in place) whose sample
        (i,j,k) sits at origin + (i,j,k) * voxel (ovn_tsdf_integrate).  With `base` (3 integers) the tensors are
        the rolling window at that base and `origin` is its anchor (ovn_tsdf_window_integrate)."""
        nx, ny, nz, org = self._tsdf_volume_args("tsdf_integrate", tsdf, weight, origin)
        b3 = None if base is None else self._int3("tsdf_integrate", "base", base)
        r = self._check(range_images, "tsdf_integrate: range_images (n,H,W)", ndim=3)
        p = self._poses64(poses)
        n, h, w = (int(v) for v in r.shape)
        if tuple(p.shape) != (n, 4, 4):
            raise _lib.OvnError("tsdf_integrate: poses must be (%d,4,4) for %d range images, got %s" % (n, n, tuple(p.shape)))
        scans = (_ptr(r), _ptr(p), n, h, w, float(fov_up), float(fov_down), float(max_range))
        if b3 is not None:
            self._call("ovn_tsdf_window_integrate", self._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, org, b3, float(voxel),
                       float(trunc), float(max_weight), *scans)
        else:
            self._call("ovn_tsdf_integrate", _ptr(tsdf), _ptr(weight), nx, ny, nz, org, float(voxel), float(trunc), float(max_weight),
                       *scans, self._stream())

    def tsdf_triangles(self, tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel: float, min_weight: float = 1.0,
                       capacity: Optional[int] = None, out: Optional[torch.Tensor] = None, base=None, box=None):
        """The zero level set of a fused volume as a triangle soup (ovn_tsdf_triangles, marching tetrahedra).  capacity=None counts
        first and then writes every triangle; otherwise at most `capacity` triangles are written (0: count only), into `out`
        ((capacity,3,3) float32) when given.  Returns (triangles (min(T, capacity),3,3) device tensor or None, T).  With `base` the
        tensors are the rolling window at that base, `origin` its anchor and box = (box_lo, box_hi) the cells to extract, by their
        low corners' lattice indices (ovn_tsdf_window_triangles)."""
        nx, ny, nz, org = self._tsdf_volume_args("tsdf_triangles", tsdf, weight, origin)
        if (base is None) != (box is None):
            raise _lib.OvnError("tsdf_triangles: base and box come together (a window), or neither (a dense volume)")
        if base is not None:
            b3 = self._int3("tsdf_triangles", "base", base)
            lo3, hi3 = self._int3("tsdf_triangles", "box_lo", box[0]), self._int3("tsdf_triangles", "box_hi", box[1])
        if out is not None:
            self._check(out, "tsdf_triangles: out (capacity,3,3)", ndim=3)
            if tuple(out.shape[1:]) != (3, 3):
                raise _lib.OvnError("tsdf_triangles: out must be a contiguous float32 (capacity,3,3) tensor on %s" % self.device)
            if capacity is None:
                capacity = int(out.shape[0])
            if int(capacity) > int(out.shape[0]):
                raise _lib.OvnError("tsdf_triangles: capacity %d exceeds the %d triangles of out" % (capacity, out.shape[0]))
        count = torch.zeros(1, dtype=torch.int64, device=self.device)

        def call(buf, cap):
            if base is not None:
                self._call("ovn_tsdf_window_triangles", self._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, org, b3, float(voxel),
                           float(min_weight), lo3, hi3, _ptr(buf), int(cap), _ptr(count))
            else:
                self._call("ovn_tsdf_triangles", _ptr(tsdf), _ptr(weight), nx, ny, nz, org, float(voxel), float(min_weight), _ptr(buf),
                           int(cap), _ptr(count), self._stream())
            return int(count.item())

        if capacity is None:
            total = call(None, 0)
            capacity = total
        elif int(capacity) < 0:
            raise _lib.OvnError("tsdf_triangles: capacity %d < 0" % capacity)
        capacity = int(capacity)
        if capacity == 0:
            return None, call(None, 0)
        buf = out if out is not None else torch.empty((capacity, 3, 3), dtype=torch.float32, device=self.device)
        total = call(buf, capacity)
        return buf[:min(total, capacity)], total

    def _direction_tables(self, proj_h: int, proj_w: int, fov_up: float, fov_down: float):
        """The four device tables of `mesh.direction_tables` for this geometry (the last geometry is kept), or four None for an
        image size the library will refuse."""
        key = (proj_h, proj_w, float(fov_up), float(fov_down))
        tabs = self._render_tables.get(key)
        if tabs is None and proj_h >= 1 and proj_w >= 1:
            from .mesh import direction_tables
            tabs = tuple(torch.from_numpy(t).to(self.device) for t in direction_tables(proj_h, proj_w, fov_up, fov_down))
            self._render_tables = {key: tabs}
        return tabs or (None,) * 4

    def tsdf_bricks(self, weight: torch.Tensor, min_weight: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The byte mask `tsdf_raycast` takes: (ceil(nz/8), ceil(ny/8), ceil(nx/8)) uint8, 1 where some sample of the 8 x 8 x 8 brick
        has weight >= min_weight (ovn_tsdf_bricks), written into `out` when given."""
        self._check(weight, "tsdf_bricks: weight (nz,ny,nx)", ndim=3)
        nz, ny, nx = (int(v) for v in weight.shape)
        shape = tuple(-(-v // 8) for v in (nz, ny, nx))
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        else:
            self._check(out, "tsdf_bricks: out", torch.uint8, shape)
        self._call("ovn_tsdf_bricks", self._stream(), _ptr(weight), nx, ny, nz, float(min_weight), _ptr(out))
        return out

    def tsdf_raycast(self, tsdf: torch.Tensor, weight: torch.Tensor, origin, voxel: float, poses, proj_h: int = 64, proj_w: int = 900,
                     fov_up: float = 3.0, fov_down: float = -25.0, min_range: float = 0.5, max_range: float = 50.0,
                     step: Optional[float] = None, min_weight: float = 1.0, bricks: Optional[torch.Tensor] = None,
                     want: Sequence[str] = ("range", "normal"), stacked_flags: Optional[Tuple[bool, ...]] = None,
                     stacked_out: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None, base=None):
        """Views of the volume tsdf / weight ((nz,ny,nx) float32 device tensors, sample (i,j,k) at origin + (i,j,k) * voxel) from
        `poses` ((n,4,4) float64 sensor-to-world, host array or device tensor): one ray per pixel marched from min_range to max_range
        in steps of `step` (default: one voxel), the first crossing from positive to non-positive tsdf is the hit (ovn_tsdf_raycast;
        DESIGN.md section 31).  `want` selects outputs among range, vertex, normal; stacked_flags = (use_depth, use_normals)
        additionally assembles the (n,H,W,C) leg input (into `stacked_out` when given).  bricks: the mask of `tsdf_bricks` for this
        weight and min_weight, or None.  out: a dict name -> contiguous float32 tensor of that output's shape (a slice along the first
        axis of a caller's buffer) to write into instead of a fresh tensor.  Returns a dict of device tensors.  With `base` the
        tensors are the rolling window at that base, `origin` its anchor and `bricks` the mask of the storage as it stands
        (ovn_tsdf_window_raycast)."""
        bad = [k for k in want if k not in _RAYCAST_OUTPUTS]
        if bad:
            raise _lib.OvnError("tsdf_raycast: no output %s (a ray-cast view has range, vertex, normal)" % bad)
        nx, ny, nz, org = self._tsdf_volume_args("tsdf_raycast", tsdf, weight, origin)
        b3 = None if base is None else self._int3("tsdf_raycast", "base", base)
        p = self._poses64(poses)
        if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
            raise _lib.OvnError("tsdf_raycast: poses must be (n,4,4), got %s" % (tuple(p.shape),))
        n = int(p.shape[0])
        proj_h, proj_w = int(proj_h), int(proj_w)
        self._check(bricks, "tsdf_raycast: bricks", torch.uint8, tuple(-(-v // 8) for v in (nz, ny, nx)), optional=True)
        out = dict(out or {})
        unknown = [k for k in out if k not in _RAYCAST_OUTPUTS]
        if unknown:
            raise _lib.OvnError("tsdf_raycast: out names %s; it takes range, vertex, normal" % unknown)
        ud = un = 0
        c = None
        if stacked_flags is not None:
            if len(stacked_flags) != 2:
                raise _lib.OvnError("tsdf_raycast: stacked_flags is (use_depth, use_normals)")
            ud, un = (int(bool(v)) for v in stacked_flags)
            c = ud + 3 * un
        bufs, stk = self._image_outputs(n, proj_h, proj_w, _RAYCAST_OUTPUTS, want, c, stacked_out, min_channels=1, out=out,
                                        what="tsdf_raycast: ")
        tabs = self._direction_tables(proj_h, proj_w, fov_up, fov_down)
        tail = (float(voxel), float(min_weight), _ptr(bricks), _ptr(p), n, proj_h, proj_w, _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]),
                _ptr(tabs[3]), float(min_range), float(max_range), float(voxel if step is None else step), _ptr(bufs.get("range")),
                _ptr(bufs.get("vertex")), _ptr(bufs.get("normal")), _ptr(stk), ud, un)
        if b3 is not None:
            self._call("ovn_tsdf_window_raycast", self._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, org, b3, *tail)
        else:
            self._call("ovn_tsdf_raycast", self._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, org, *tail)
        if stk is not None:
            bufs["stacked"] = stk
        return bufs

    def tsdf_window_shift(self, tsdf: torch.Tensor, weight: torch.Tensor, old_base, new_base) -> None:
        """The rolling window tsdf / weight moves from old_base to new_base (3 integers each): the slots whose samples leave become
        (tsdf 1, weight 0) for the samples that enter, nothing else is written (ovn_tsdf_window_shift)."""
        nx, ny, nz, _ = self._tsdf_volume_args("tsdf_window_shift", tsdf, weight, (0.0, 0.0, 0.0))
        ob, nb = self._int3("tsdf_window_shift", "old_base", old_base), self._int3("tsdf_window_shift", "new_base", new_base)
        self._call("ovn_tsdf_window_shift", self._stream(), _ptr(tsdf), _ptr(weight), nx, ny, nz, ob, nb)

    def icp_register(self, vertex: torch.Tensor, normal: torch.Tensor, rng: torch.Tensor, src_idx: torch.Tensor,
                     tgt_idx: torch.Tensor, init_pose: torch.Tensor, iterations: int = 20, max_dist: float = 2.0,
                     cos_min: float = 0.8, huber: float = 0.2, min_inliers: int = 64, fov_up: float = 3.0, fov_down: float = -25.0,
                     max_range: float = 50.0, want_system: bool = False):
        """Projective point-to-plane ICP on `project`'s images, every pair in one launch (`ovn_icp_register`).  vertex (n,H,W,4),
        normal (n,H,W,3), rng (n,H,W) f32; src_idx / tgt_idx (P) int32; init_pose (P,4,4) f64, source-frame points into the target
        frame.  Returns (pose (P,4,4) f64, stats (P,8) f64: status, passes solved, inliers, valid source pixels, rms, |v| and
        |omega| of the last step, 0) as device tensors, plus the first pass's normal equations (P,28) with want_system=True."""
        for t, what, dt in ((vertex, "vertex", torch.float32), (normal, "normal", torch.float32), (rng, "range", torch.float32),
                            (src_idx, "src_idx", torch.int32), (tgt_idx, "tgt_idx", torch.int32),
                            (init_pose, "init_pose", torch.float64)):
            self._check(t, "icp_register(): " + what, dt)
        if rng.dim() != 3:
            raise _lib.OvnError("icp_register(): range must be (n, H, W), got %s" % (tuple(rng.shape),))
        n, h, w = (int(v) for v in rng.shape)
        if tuple(vertex.shape) != (n, h, w, 4) or tuple(normal.shape) != (n, h, w, 3):
            raise _lib.OvnError("icp_register(): vertex %s / normal %s do not match range %s"
                                % (tuple(vertex.shape), tuple(normal.shape), tuple(rng.shape)))
        p = int(src_idx.numel())
        if int(tgt_idx.numel()) != p or tuple(init_pose.shape) != (p, 4, 4):
            raise _lib.OvnError("icp_register(): %d source indices, %d target indices, init_pose %s"
                                % (p, int(tgt_idx.numel()), tuple(init_pose.shape)))
        pose = torch.empty((p, 4, 4), dtype=torch.float64, device=self.device)
        stats = torch.empty((p, 8), dtype=torch.float64, device=self.device)
        system = torch.empty((p, 28), dtype=torch.float64, device=self.device) if want_system else None
        self._call("ovn_icp_register", _ptr(vertex), _ptr(normal), _ptr(rng), n, h, w, float(fov_up), float(fov_down), float(max_range),
                   _ptr(src_idx), _ptr(tgt_idx), p, _ptr(init_pose), int(iterations), float(max_dist), float(cos_min), float(huber),
                   int(min_inliers), _ptr(pose), _ptr(stats), _ptr(system), self._stream())
        return (pose, stats, system) if want_system else (pose, stats)

    # -- Monte Carlo localization (csrc/mcl.hip) -------------------------------------------------------
    def _mcl_particles(self, particles: torch.Tensor, what: str = "particles") -> int:
        self._check(particles, what)
        if particles.dim() != 2 or particles.shape[1] != 4:
            raise _lib.OvnError("%s must be (P, 4) rows x, y, theta, w; got %s" % (what, tuple(particles.shape)))
        return int(particles.shape[0])

    def mcl_predict(self, particles: torch.Tensor, odom, sigma, seed: int, step: int, cell_frame: torch.Tensor, origin, resolution: float,
                    nx: int, ny: int, n_frames: int, particle_frame: Optional[torch.Tensor] = None,
                    frame_slot: Optional[torch.Tensor] = None, frame_list: Optional[torch.Tensor] = None,
                    record: Optional[torch.Tensor] = None):
        """Motion update of the (P,4) particles IN PLACE with Philox noise, their map frames, and the ascending list of the distinct
        frames (`ovn_mcl_predict`).  odom = (dx, dy, dtheta) in the robot frame, sigma = (sigma_x, sigma_y, sigma_theta), origin =
        (origin_x, origin_y); cell_frame (ny*nx) int32.  Returns (particle_frame (P), frame_slot (M), frame_list (M), record (4)) int32;
        record = {U, particles off the map, 0, 1} may be a pinned host tensor (the caller synchronises before reading it)."""
        p = self._mcl_particles(particles)
        nx, ny, m = int(nx), int(ny), int(n_frames)
        i32 = torch.int32
        self._check(cell_frame, "cell_frame", i32, numel=max(nx, 0) * max(ny, 0))
        if particle_frame is None:
            particle_frame = torch.empty(p, dtype=torch.int32, device=self.device)
        if frame_slot is None:
            frame_slot = torch.empty(max(m, 0), dtype=torch.int32, device=self.device)
        if frame_list is None:
            frame_list = torch.empty(max(m, 0), dtype=torch.int32, device=self.device)
        if record is None:
            record = torch.empty(4, dtype=torch.int32, device=self.device)
        self._check(particle_frame, "particle_frame", i32, numel=p)
        self._check(frame_slot, "frame_slot", i32, numel=max(m, 0))
        self._check(frame_list, "frame_list", i32, numel=max(m, 0))
        self._check(record, "record", i32, numel=4, pinned_ok=True)
        dx, dy, dth = (float(v) for v in odom)
        sx, sy, sth = (float(v) for v in sigma)
        self._call("ovn_mcl_predict", _ptr(particles), p, dx, dy, dth, sx, sy, sth, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1),
                   _ptr(cell_frame), float(origin[0]), float(origin[1]), float(resolution), nx, ny, m, _ptr(particle_frame),
                   _ptr(frame_slot), _ptr(frame_list), _ptr(record), self._stream())
        return particle_frame, frame_slot, frame_list, record

    def mcl_update(self, particles: torch.Tensor, particle_frame: torch.Tensor, frame_slot: torch.Tensor, frame_yaw: torch.Tensor,
                   overlap: Optional[torch.Tensor], yaw: Optional[torch.Tensor], sigma_yaw: float, eps_yaw: float, overlap_min: float,
                   estimate: Optional[torch.Tensor] = None, want_spread: bool = False):
        """Observation-model weights IN PLACE from the sweep's scores over frame_list[:U] (overlap (U) f32, yaw (U) int32; both None
        when U == 0), the exact power-of-two rescale and the estimate (`ovn_mcl_update`): a (8,) float64 device tensor {status,
        sum w, N_eff, mean x, mean y, circular mean heading, position of the first maximum weight, particles on the map}; with
        want_spread=True also the weighted rms distance from the mean position, a (1,) float64 device tensor."""
        p = self._mcl_particles(particles)
        m = int(frame_slot.numel())
        self._check(particle_frame, "particle_frame", torch.int32, numel=p)
        self._check(frame_slot, "frame_slot", torch.int32)
        self._check(frame_yaw, "frame_yaw", torch.float32, numel=m)
        if (overlap is None) != (yaw is None):
            raise _lib.OvnError("mcl_update(): overlap and yaw must be given together")
        u = 0
        if overlap is not None:
            u = int(overlap.numel())
            self._check(overlap, "overlap", torch.float32)
            self._check(yaw, "yaw", torch.int32, numel=u)
        if estimate is None:
            estimate = torch.empty(8, dtype=torch.float64, device=self.device)
        self._check(estimate, "estimate", torch.float64, numel=8)
        spread = torch.empty(1, dtype=torch.float64, device=self.device) if want_spread else None
        self._call("ovn_mcl_update", _ptr(particles), p, _ptr(particle_frame), _ptr(frame_slot), _ptr(frame_yaw), m,
                   _ptr(overlap) if u else None, _ptr(yaw) if u else None, u, float(sigma_yaw), float(eps_yaw), float(overlap_min),
                   _ptr(estimate), _ptr(spread), self._stream())
        return (estimate, spread) if want_spread else estimate

    def mcl_resample(self, particles: torch.Tensor, seed: int, step: int, n_out: Optional[int] = None,
                     out: Optional[torch.Tensor] = None, ancestors: Optional[torch.Tensor] = None,
                     record: Optional[torch.Tensor] = None):
        """Systematic resampling, exact in integers (`ovn_mcl_resample`): n_out (default P) copies with weight 1 into `out`, which must
        not overlap `particles`.  Returns (out (n_out,4) f32, ancestors (n_out) int32, record (4) int32 = {status, written, 0, 1});
        status 1: no positive weight, nothing but the record is written.  `record` may be a pinned host tensor."""
        p = self._mcl_particles(particles)
        n_out = p if n_out is None else int(n_out)
        if out is None:
            out = torch.empty((max(n_out, 0), 4), dtype=torch.float32, device=self.device)
        if self._mcl_particles(out, "out") != n_out:
            raise _lib.OvnError("mcl_resample(): out holds %d particles, n_out is %d" % (out.shape[0], n_out))
        if ancestors is None:
            ancestors = torch.empty(max(n_out, 0), dtype=torch.int32, device=self.device)
        if record is None:
            record = torch.empty(4, dtype=torch.int32, device=self.device)
        self._check(ancestors, "ancestors", torch.int32, numel=max(n_out, 0))
        self._check(record, "record", torch.int32, numel=4, pinned_ok=True)
        self._call("ovn_mcl_resample", _ptr(particles), p, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), _ptr(out), n_out,
                   _ptr(ancestors), _ptr(record), self._stream())
        return out, ancestors, record

    def projection_angles(self, points: torch.Tensor, proj_h: int = 64, proj_w: int = 900, fov_up: float = 3.0,
                          fov_down: float = -25.0, max_range: float = 50.0):
        """(yaw, pitch, pixel) of every point of an (n, 4) float32 device tensor as the projection kernel evaluates them
        (utils.py:75-104; pixel = -1 for points the range filter drops) -- validation entry, include/ovn_hip.h."""
        self._check(points, "projection_angles(): points (n, 4)", ndim=2)
        if points.shape[1] != 4:
            raise _lib.OvnError("projection_angles(): points must be a contiguous (n, 4) float32 tensor on %s" % self.device)
        n = points.shape[0]
        yaw = torch.empty(n, dtype=torch.float32, device=self.device)
        pitch = torch.empty(n, dtype=torch.float32, device=self.device)
        pix = torch.empty(n, dtype=torch.int32, device=self.device)
        self._call("ovn_projection_angles", _ptr(points), n, proj_h, proj_w, float(fov_up), float(fov_down), float(max_range), _ptr(yaw),
                   _ptr(pitch), _ptr(pix), self._stream())
        return yaw, pitch, pix

    def debug_head_activations(self, n: int):
        """(o2 (n,G,G,128), o3 (n,G-2,G-2,256)), G = feat_w // 15, left in scratch by the last heads() call -- test hook.
        The fp32 kernels (head precision 'f32', or any precision at feat_w != 360) keep them only for a heads() call that ran as
        one chunk; the split-operand modes keep those of the call's first sub-chunk."""
        g = self._fw // 15
        o2 = torch.empty((n, g, g, 128), dtype=torch.float32, device=self.device)
        o3 = torch.empty((n, g - 2, g - 2, 256), dtype=torch.float32, device=self.device)
        self._call("ovn_debug_head_activations", n, _ptr(o2), _ptr(o3), self._stream())
        return o2, o3

    def set_head_pipeline(self, chunk_pairs: int = 1024, sub_chunk_pairs: int = 0, streams: int = 1, yaw_on_side_stream: bool = False):
        """Launch structure of the head calls (include/ovn_hip.h: ovn_set_head_pipeline); results do not depend on it."""
        self._call("ovn_set_head_pipeline", int(chunk_pairs), int(sub_chunk_pairs), int(streams), int(bool(yaw_on_side_stream)))

    def head_pipeline(self):
        """(chunk_pairs, sub_chunk_pairs, streams, yaw_on_side_stream) currently in effect."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
        self._call("ovn_get_head_pipeline", C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return int(a.value), int(b.value), int(c.value), bool(d.value)

    def set_head_precision(self, mode: str) -> None:
        """Arithmetic of the Delta-head contractions (fp32 storage and accumulation in both modes):
        'f16x3' (default) = scaled 3-term fp16 split on the fp16 matrix cores (22 significand bits per operand: the error of an
        fp32 evaluation), 'f32' = fp32 matrix cores (bit-for-bit an fp32 FMA chain, 1/16 of the rate), 'bf16x3' = exact 3-term bf16
        split on the bf16 matrix cores (operands at least as wide as fp32: 24 significand bits; include/ovn_hip.h).
        At a feature width other than 360 every mode runs the exact fp32 heads of the 'f32' mode (delta_head.hip / corr_head.hip) by default: the
        tuned split-operand kernels are tiled to 24 column groups of 15 and to the 360-point DFT, and fp32 is the reference's own
        arithmetic.  With `set_head_width_split(True)` the 'f16x3' mode runs DeltaLayer + c_conv1 + c_conv2 there in its own
        arithmetic on the runtime-width kernels of delta_head_w_f16x3.hip (c_conv3, Dense and the yaw head stay fp32); 'f32' and
        'bf16x3' keep the fp32 kernels.  The mode is recorded either way (and the leg follows its own precision setting)."""
        table = {"f32": 0, "f16x3": 1, "bf16x3": 2}
        if mode not in table:
            raise ValueError("head precision must be one of %s" % sorted(table))
        self._call("ovn_set_head_precision", table[mode])
        self.head_precision = mode

    def set_head_width_split(self, on: bool) -> None:
        """Delta head at a feature width other than 360 (conv1size 15): False (default) = exact fp32 in every head precision, True =
        head precision 'f16x3' runs DeltaLayer + c_conv1 + c_conv2 in the scaled 3-term fp16 split (delta_head_w_f16x3.hip),
        several times the fp32 rate at the error of the 360 path.  No effect at 360 columns or in the other head precisions."""
        self._call("ovn_set_head_width_split", 1 if on else 0)
        got = C.c_int()
        self._call("ovn_get_head_width_split", C.byref(got))
        self.head_width_split = bool(got.value)

    def set_corr_normalization(self, mode: str) -> None:
        """Normalisation of the correlation head's inputs, NormalizedCorrelation2D(normalize=mode): 'none' (default, what
        generateCorrelationHead builds), 'euclidean', 'scaling' or 'standardization' -- per (volume, channel) over the 360 columns,
        statistics in fp64, each element rounded once to fp32 (include/ovn_hip.h: ovn_set_corr_normalization).  Spectra from
        `spectrum` are valid for the mode they were built under; the Delta head is not affected."""
        if not isinstance(mode, str) or mode not in W.CORR_NORMALIZE_MODES:
            raise ValueError("correlation normalisation must be one of %s" % sorted(W.CORR_NORMALIZE_MODES))
        self._call("ovn_set_corr_normalization", W.CORR_NORMALIZE_MODES[mode])

    @property
    def corr_normalization(self) -> str:
        """The normalisation mode the library context holds (ovn_get_corr_normalization)."""
        m = C.c_int(-1)
        self._call("ovn_get_corr_normalization", C.byref(m))
        return {v: k for k, v in W.CORR_NORMALIZE_MODES.items()}[m.value]

    def set_head_compaction(self, on: bool) -> None:
        """1-vs-N sweeps drop the query's dead feature channels (zero in all 360 columns) from the Delta head's contraction (default on;
        exact -- include/ovn_hip.h: ovn_set_head_compaction).  Off: every pair walks all 128 channels, as indexed pairs always do."""
        self._call("ovn_set_head_compaction", int(bool(on)))
        self.head_compaction = bool(on)

    def head_walk_stats(self) -> dict:
        """The K walk the Delta head's contraction took in the most recent 1-vs-N sweep (`ovn_head_walk_stats`): per column-group pair
        the slices of 32 channels its live channels need (`slices_per_group_pair`, 12 entries), the query's live channels, and
        `k_walk_frac` = the MFMAs the kernel issued / those of the 128-channel walk: wave w of the contraction kernel holds column
        groups 3 w .. 3 w + 2 and skips a slice when none of them walks it; a last slice of <= 16 live channels is packed tap-major
        into `packed_last_slice_steps` steps instead of 15 (csrc/delta_head_f16x3.hip)."""
        out = (C.c_int32 * 16)()
        self._call("ovn_head_walk_stats", out, self._stream())
        spp = [int(out[2 + p]) for p in range(12)]
        per_wave = [max(spp[(3 * w) // 2], spp[(3 * w + 2) // 2]) for w in range(8)]
        nsm, tail = int(out[0]), int(out[15])

        def steps(ns):      # MFMA steps of a walk of ns slices: 15 each, the packed last slice (if it is among them) `tail`
            return 15 * ns - ((15 - tail) if (tail and ns == nsm) else 0)
        return {"max_slices": nsm, "live_channels": int(out[1]), "slices_per_group_pair": spp, "packed_last_slice_steps": tail,
                "compacted": bool(out[14]), "k_walk_frac": sum(steps(n) for n in per_wave) / (8 * 60.0),
                "k_walk_frac_time": steps(nsm) / 60.0}

    def set_projection_trig(self, mode: str) -> None:
        """Which float32 `np.arctan2` / `np.arcsin` (utils.py:86-87) `project` reproduces: 'numpy_avx512' (default: NumPy >= 1.22 on an
        AVX512_SKX x86-64 host -- Intel SVML, bit for bit; the machine the reference's shipped .npy files were made on) or 'rounded'
        (the correctly rounded float32 results: NumPy on hosts whose float32 loops call a correctly rounded libm)."""
        table = {"numpy_avx512": 0, "rounded": 1}
        if mode not in table:
            raise ValueError("projection trig must be one of %s" % sorted(table))
        self._call("ovn_set_projection_trig", table[mode])
        self.projection_trig = mode

    def set_leg_precision(self, mode: str) -> None:
        """Arithmetic of the leg convolutions: 'f16x3' (default, as above) or 'f32' (fp32 matrix cores)."""
        table = {"f32": 0, "f16x3": 1}
        if mode not in table:
            raise ValueError("leg precision must be one of %s" % sorted(table))
        self._call("ovn_set_leg_precision", table[mode])
        self.leg_precision = mode

    PROFILE_KINDS = ("leg_conv", "corr_head", "delta_c12", "c_conv3", "dense_sigmoid", "projection", "spectrum",
                     "corr_spectral", "delta_prep", "delta_c2")

    def profile_begin(self) -> None:
        self._call("ovn_profile_begin")

    def profile_end(self):
        """{kind: (total_ms, launches)} measured with HIP events on the launch stream."""
        ms = (C.c_double * len(self.PROFILE_KINDS))()
        cnt = (C.c_int64 * len(self.PROFILE_KINDS))()
        self._call("ovn_profile_end", ms, cnt)
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.PROFILE_KINDS)}

    # -- pose-graph optimization (ovn_pose_graph_*) -------------------------------------------
    POSE_GRAPH_RECORD = ("cost", "bad_edges", "cholesky_failures", "grad_max", "iterations", "relative_residual", "converged",
                         "breakdown", "rz", "rz0", "alpha", "beta", "delta_max")
    POSE_GRAPH_PRECONDITIONERS = {"jacobi": 0, "chain": 1}
    POSE_GRAPH_LOOPS = 2                       # OVN_POSE_GRAPH_LOOPS: served by the ovn_pose_graph_*_loops entries
    POSE_GRAPH_MAX_LOOPS = 256                 # OVN_POSE_GRAPH_MAX_LOOPS

    def pose_graph_buffers(self, n_nodes: int, n_edges: int, chain: bool = False, loops: int = 0) -> Dict[str, torch.Tensor]:
        """Every device buffer the pose-graph calls write, sized for n_nodes and n_edges: res, chi, weight, jac, blocks, grad, diag,
        dinv, chain (when asked), delta, ws (ovn_pose_graph_workspace_bytes) and record.  loops=L > 0 adds chain and `loops`
        (ovn_pose_graph_loops_bytes) for the chain-plus-loops inverse of a graph whose last L edges are its loop edges."""
        n, e = int(n_nodes), int(n_edges)
        if int(loops) > 0:
            nl = int(loops)
            lbytes = int(self.lib.ovn_pose_graph_loops_bytes(n, nl))
            if lbytes <= 0 or e != n - 1 + nl:
                raise _lib.OvnError("pose graph of %d nodes, %d edges and %d loop edges: the chain-plus-loops inverse takes 1..%d loop "
                                    "edges after the %d chain edges" % (n, e, nl, self.POSE_GRAPH_MAX_LOOPS, n - 1))
            b = self.pose_graph_buffers(n, e, chain=True)
            b["loops"] = torch.zeros(lbytes // 8, dtype=torch.float64, device=self.device)
            return b
        nbytes = int(self.lib.ovn_pose_graph_workspace_bytes(n, e))
        if nbytes <= 0:
            raise _lib.OvnError("pose graph of %d nodes and %d edges is outside the library's limits" % (n, e))
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=self.device)
        b = dict(res=z(e, 6), chi=z(e), weight=z(e), jac=z(e, 2, 6, 6), blocks=z(e, 3, 6, 6), grad=z(n, 6), diag=z(n, 6, 6),
                 dinv=z(n, 6, 6), delta=z(n, 6), ws=z(nbytes // 8), record=z(16))
        if chain:
            b["chain"] = z(max(n - 1, 0), 2, 6, 6)
        return b

    def pose_graph_linearize(self, poses, fixed, edge_ij, meas, info, node_ptr, node_edge, huber: float, buf: Dict[str, torch.Tensor],
                             jacobians: bool = True, record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Residuals, weights and cost of the edges at `poses` into buf's res, chi, weight, and with jacobians=True the Jacobians,
        Hessian blocks, gradient, diagonal blocks, their inverses and (when buf has "chain") the chain preconditioner's terms
        (ovn_pose_graph_linearize).  Returns the record tensor (buf["record"] unless another is given)."""
        f64, n, e = torch.float64, int(poses.shape[0]), int(edge_ij.shape[0])
        for name, t, dt, shape in (("poses", poses, f64, (n, 4, 4)), ("fixed", fixed, torch.uint8, (n,)),
                                   ("edge_ij", edge_ij, torch.int32, (e, 2)), ("meas", meas, f64, (e, 4, 4)), ("info", info, f64, (e, 6, 6)),
                                   ("node_ptr", node_ptr, torch.int32, (n + 1,)), ("node_edge", node_edge, torch.int32, (2 * e,))):
            self._check(t, "pose_graph_linearize: " + name, dt, shape)
        rec = self._check(buf["record"] if record is None else record, "pose_graph_linearize: record", f64, (16,))
        for k, s in (("res", (e, 6)), ("chi", (e,)), ("weight", (e,)), ("jac", (e, 2, 6, 6)), ("blocks", (e, 3, 6, 6)), ("grad", (n, 6)),
                     ("diag", (n, 6, 6)), ("dinv", (n, 6, 6))):
            self._check(buf[k], "pose_graph_linearize: buf[%r]" % k, f64, s)
        ch = self._check(buf.get("chain"), "pose_graph_linearize: buf['chain']", f64, (max(n - 1, 0), 2, 6, 6), optional=True)
        j = (lambda k: _ptr(buf[k])) if jacobians else (lambda k: None)
        self._call("ovn_pose_graph_linearize", self._stream(), _ptr(poses), _ptr(fixed), n, _ptr(edge_ij), _ptr(meas), _ptr(info), e,
                   _ptr(node_ptr), _ptr(node_edge), float(huber), _ptr(buf["res"]), _ptr(buf["chi"]), _ptr(buf["weight"]), j("jac"),
                   j("blocks"), j("grad"), j("diag"), j("dinv"), _ptr(ch) if jacobians else None, _ptr(buf["ws"]), _ptr(rec))
        return rec

    def pose_graph_solve(self, fixed, edge_ij, node_ptr, node_edge, buf: Dict[str, torch.Tensor], preconditioner="jacobi",
                         lam: float = 0.0, rtol: float = 1e-8, first_iteration: int = 0, iterations: int = 32) -> torch.Tensor:
        """Enqueues `iterations` PCG iterations on the linearization in `buf` (ovn_pose_graph_solve); delta in buf["delta"], state in
        buf["ws"], status in the returned record tensor.  Never waits for the GPU."""
        n, e = int(fixed.shape[0]), int(edge_ij.shape[0])
        system = (self._stream(), _ptr(fixed), n, _ptr(edge_ij), e, _ptr(node_ptr), _ptr(node_edge), _ptr(buf["blocks"]), _ptr(buf["grad"]),
                  _ptr(buf["diag"]), _ptr(buf["dinv"]), _ptr(buf.get("chain")))
        run = (float(lam), float(rtol), int(first_iteration), int(iterations), _ptr(buf["delta"]), _ptr(buf["ws"]), _ptr(buf["record"]))
        if preconditioner in ("loops", self.POSE_GRAPH_LOOPS):
            lp = self._pg_loops(buf, n, e - (n - 1), "pose_graph_solve")
            self._call("ovn_pose_graph_solve_loops", *system, _ptr(lp), e - (n - 1), *run)
            return buf["record"]
        kind = self.POSE_GRAPH_PRECONDITIONERS.get(preconditioner, preconditioner)
        if not isinstance(kind, int):
            raise _lib.OvnError("pose_graph_solve: no preconditioner %r (jacobi, chain, loops)" % (preconditioner,))
        self._call("ovn_pose_graph_solve", *system, kind, *run)
        return buf["record"]

    def _pg_loops(self, buf: Dict[str, torch.Tensor], n: int, n_loops: int, what: str) -> torch.Tensor:
        nbytes = int(self.lib.ovn_pose_graph_loops_bytes(n, n_loops))
        if nbytes <= 0:
            raise _lib.OvnError("%s: the chain-plus-loops inverse takes 1..%d loop edges after the chain, got %d"
                                % (what, self.POSE_GRAPH_MAX_LOOPS, n_loops))
        if buf.get("chain") is None or buf.get("loops") is None:
            raise _lib.OvnError("%s: the buffers were not made with loops=%d (pose_graph_buffers)" % (what, n_loops))
        return self._check(buf["loops"], "%s: buf['loops']" % what, torch.float64, (nbytes // 8,))

    def pose_graph_loops_prepare(self, poses, edge_ij, info, buf: Dict[str, torch.Tensor],
                                 record: Optional[torch.Tensor] = None, stages: int = 7) -> torch.Tensor:
        """Gamma, C, the spans, S and its Cholesky factor of the chain-plus-loops inverse into buf["loops"], from the linearization
        (with Jacobians) that `buf` holds for `poses` (ovn_pose_graph_loops_prepare).  Returns the record tensor: slot 13 counts
        failed pivots, slot 14 the loop edges left out.  stages: 1 = scan, 2 = assembly, 4 = factorization, summed (a benchmark's knob)."""
        f64, n, e = torch.float64, int(poses.shape[0]), int(edge_ij.shape[0])
        what = "pose_graph_loops_prepare: "
        self._check(poses, what + "poses", f64, (n, 4, 4))
        self._check(edge_ij, what + "edge_ij", torch.int32, (e, 2))
        self._check(info, what + "info", f64, (e, 6, 6))
        lp = self._pg_loops(buf, n, e - (n - 1), "pose_graph_loops_prepare")
        self._check(buf["weight"], what + "buf['weight']", f64, (e,))
        self._check(buf["jac"], what + "buf['jac']", f64, (e, 2, 6, 6))
        self._check(buf["chain"], what + "buf['chain']", f64, (n - 1, 2, 6, 6))
        rec = self._check(buf["record"] if record is None else record, what + "record", f64, (16,))
        self._call("ovn_pose_graph_loops_prepare", self._stream(), _ptr(poses), n, _ptr(edge_ij), _ptr(info), _ptr(buf["weight"]),
                   _ptr(buf["jac"]), e, e - (n - 1), _ptr(buf["chain"]), int(stages), _ptr(lp), _ptr(rec))
        return rec

    def pose_graph_loops_views(self, buf: Dict[str, torch.Tensor], n_nodes: int, n_loops: int) -> Dict[str, torch.Tensor]:
        """Views into buf["loops"] (ovn_pose_graph_loops_layout): gamma (N,6,6), C (L,6,6), winv (L,6,6), span (L,4), S (sp,sp),
        factor (sp,sp), and the integers block and sp."""
        n, nl = int(n_nodes), int(n_loops)
        lay = (C.c_int64 * 8)()
        _lib.check(self.lib.ovn_pose_graph_loops_layout(n, nl, lay), "ovn_pose_graph_loops_layout")
        b, sp = int(lay[0]), int(lay[1])
        lp = self._pg_loops(buf, n, nl, "pose_graph_loops_views")
        v = lambda k, *s: lp[int(lay[k]):int(lay[k]) + int(np.prod(s))].view(*s)
        return dict(block=b, sp=sp, gamma=v(2, n, 6, 6), C=v(3, nl, 6, 6), winv=v(4, nl, 6, 6), span=v(5, nl, 4), S=v(6, sp, sp),
                    factor=v(7, sp, sp))

    def pose_graph_precondition(self, vec: torch.Tensor, buf: Dict[str, torch.Tensor], preconditioner="jacobi", lam: float = 0.0,
                                out: Optional[torch.Tensor] = None, node_ptr: Optional[torch.Tensor] = None,
                                node_edge: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out (N,6) = M^-1 vec (N,6) for the preconditioner of the linearization in `buf` (ovn_pose_graph_precondition); "loops"
        also takes the graph's incidence list node_ptr, node_edge (ovn_pose_graph_precondition_loops; lam is not used: the inverse
        is that of the undamped Hessian)."""
        n = int(vec.shape[0])
        what = "pose_graph_precondition: "
        self._check(vec, what + "vec", torch.float64, (n, 6))
        out = torch.zeros_like(vec) if out is None else self._check(out, what + "out", torch.float64, (n, 6))
        if preconditioner in ("loops", self.POSE_GRAPH_LOOPS):
            self._check(node_ptr, what + "node_ptr", torch.int32, (n + 1,))
            self._check(node_edge, what + "node_edge", torch.int32)
            e = int(node_edge.shape[0]) // 2
            lp = self._pg_loops(buf, n, e - (n - 1), "pose_graph_precondition")
            self._call("ovn_pose_graph_precondition_loops", self._stream(), n, e, e - (n - 1), _ptr(node_ptr), _ptr(node_edge),
                       _ptr(buf["chain"]), _ptr(lp), _ptr(vec), _ptr(out), _ptr(buf["ws"]))
            return out
        kind = self.POSE_GRAPH_PRECONDITIONERS.get(preconditioner, preconditioner)
        if not isinstance(kind, int):
            raise _lib.OvnError("pose_graph_precondition: no preconditioner %r (jacobi, chain, loops)" % (preconditioner,))
        self._call("ovn_pose_graph_precondition", self._stream(), n, kind, float(lam), _ptr(buf.get("dinv")), _ptr(buf.get("chain")),
                   _ptr(vec), _ptr(out), _ptr(buf["ws"]))
        return out

    POSE_GRAPH_COV_FRAMES = {"local": 0, "position": 1}      # OVN_POSE_GRAPH_COV_LOCAL, OVN_POSE_GRAPH_COV_POSITION

    def pose_graph_marginals_bytes(self, n_nodes: int, n_loops: int, n_query: int) -> int:
        """The size of the workspace of `pose_graph_marginals` (ovn_pose_graph_marginals_bytes); 0 outside the limits."""
        return int(self.lib.ovn_pose_graph_marginals_bytes(int(n_nodes), int(n_loops), int(n_query)))

    def pose_graph_marginals(self, poses: torch.Tensor, buf: Dict[str, torch.Tensor], node_ids: torch.Tensor, n_loops: int,
                             frame: str = "position", cov: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                             record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """cov (K,6,6): the marginal covariances of the nodes node_ids (K) int32 from the linearization (with chain) that `buf` holds
        for `poses` and, for n_loops >= 1, the `pose_graph_loops_prepare` after it (ovn_pose_graph_marginals).
        frame: "local" (the optimizer's delta_k) or "position" (position and rotation vector in the world).  Slot 15 of the record
        counts the ids outside [0, N), whose blocks are NaN; slot 7 is set, and cov left as it was, when a pivot had failed."""
        n, nl = int(poses.shape[0]), int(n_loops)
        f64 = torch.float64
        what = "pose_graph_marginals: "
        if frame not in self.POSE_GRAPH_COV_FRAMES:
            raise _lib.OvnError("pose_graph_marginals: no frame %r (local, position)" % (frame,))
        self._check(poses, what + "poses", f64, (n, 4, 4))
        ids = self._check(node_ids, what + "node_ids", torch.int32)
        if ids.dim() != 1 or ids.shape[0] < 1:
            raise _lib.OvnError("pose_graph_marginals: node_ids must be (K,) with K >= 1, got %s" % (tuple(ids.shape),))
        k = int(ids.shape[0])
        nbytes = self.pose_graph_marginals_bytes(n, nl, k)
        if nbytes == 0:
            raise _lib.OvnError("pose_graph_marginals: %d nodes, %d loop edges, %d queried nodes are outside the limits" % (n, nl, k))
        self._check(buf.get("chain"), what + "buf['chain']", f64, (n - 1, 2, 6, 6))
        lp = self._pg_loops(buf, n, nl, "pose_graph_marginals") if nl > 0 else None
        rec = self._check(buf["record"] if record is None else record, what + "record", f64, (16,))
        cov = torch.zeros((k, 6, 6), dtype=f64, device=self.device) if cov is None else self._check(cov, what + "cov", f64, (k, 6, 6))
        ws = torch.empty(nbytes // 8, dtype=f64, device=self.device) if ws is None else self._check(ws, what + "ws", f64)
        if ws.numel() * 8 < nbytes:
            raise _lib.OvnError("pose_graph_marginals: ws holds %d bytes, %d are needed" % (ws.numel() * 8, nbytes))
        self._call("ovn_pose_graph_marginals", self._stream(), _ptr(poses), n, n - 1 + nl, nl, _ptr(buf["chain"]), _ptr(lp), _ptr(ids), k,
                   self.POSE_GRAPH_COV_FRAMES[frame], _ptr(cov), _ptr(ws), _ptr(rec))
        return cov

    def pose_graph_retract(self, poses: torch.Tensor, fixed: torch.Tensor, buf: Dict[str, torch.Tensor],
                           out: Optional[torch.Tensor] = None, record: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out (N,4,4) = T_i Exp(delta_i) with delta = buf["delta"] (ovn_pose_graph_retract); |delta|_inf goes to slot 12 of the record."""
        n = int(poses.shape[0])
        what = "pose_graph_retract: "
        self._check(poses, what + "poses", torch.float64, (n, 4, 4))
        self._check(fixed, what + "fixed", torch.uint8, (n,))
        self._check(buf["delta"], what + "buf['delta']", torch.float64, (n, 6))
        out = torch.empty_like(poses) if out is None else self._check(out, what + "out", torch.float64, (n, 4, 4))
        if out.data_ptr() == poses.data_ptr():
            raise _lib.OvnError("pose_graph_retract: out must not be poses")
        rec = buf["record"] if record is None else record
        self._call("ovn_pose_graph_retract", self._stream(), _ptr(poses), _ptr(fixed), _ptr(buf["delta"]), n, _ptr(out), _ptr(buf["ws"]),
                   _ptr(rec))
        return out

    def selftest(self) -> None:
        self._call("ovn_selftest")

    def workspace_bytes(self) -> int:
        return int(self.lib.ovn_workspace_bytes(self._h))


class QueryAhead:
    """Leg + spectrum of the NEXT query scan on a second library context and HIP stream, beside the head kernels that the caller's
    stream is running for the CURRENT query (a recorded sequence, or a live one whose next scan has arrived: the 1-vs-N sweep of
    `Infer.infer_multiple`, infer.py:162-203, spends 0.15 ms of its ~5.6 ms per query in a single-scan leg whose five kernels are a
    handful of workgroups deep in their own latency and leave the GPU idle).  A context owns its scratch, hence the second context;
    features and spectra are double-buffered: the pair handed out by take() may be read by work enqueued on the current stream
    up to the NEXT submit() / take() call (that call records, on the current stream, the event the slot's next overwrite waits
    for -- whatever `wait_current` says); work enqueued later must read its own copy.

        qa = QueryAhead(engine, weights, model_cfg)
        qa.submit(image_0)
        for k in range(n):
            if k + 1 < n: qa.submit(image_{k+1})          # enqueued on the side stream, returns at once
            fv, spec = qa.take()                          # the current stream now waits for query k's features (not the host)
            engine.heads(cands, fv, spec_l=cand_spec, spec_r=spec, dcache_l=cand_dc)

    Same kernels, same bits as `engine.leg` / `engine.spectrum` on the caller's stream (tests/test_gpu_parity.py)."""

    def __init__(self, engine: OvnEngine, weights: Dict[str, np.ndarray], model_cfg: Optional[dict] = None,
                 with_delta_cache: bool = False):
        """with_delta_cache: also compute the query's Delta cache row (`take_all`), for callers that cache every query as a future
        candidate (Infer.infer_multiple)."""
        self.main = engine
        self.side = OvnEngine(engine.in_h, engine.in_w, engine.in_c, device=engine.device_index)
        self.side.load_weights(weights, model_cfg)
        self.side.set_leg_precision(engine.leg_precision)
        self.side.set_head_precision(engine.head_precision)       # the spectrum kernel follows the head arithmetic
        self.side.set_head_width_split(engine.head_width_split)
        self.side.set_projection_trig(engine.projection_trig)     # (the look-ahead of Infer projects raw scans in this context)
        self.side.set_corr_normalization(engine.corr_normalization)   # the query spectrum is that of the normalised volume
        dev = engine.device
        with torch.cuda.device(dev):
            self.stream = torch.cuda.Stream(device=dev)
            self._fv = [torch.empty((1, self.side.feat_w, FEAT_C), dtype=torch.float32, device=dev) for _ in range(2)]
            # no spectrum at a feature width other than 360: take() hands out (volume, None), the look-ahead is the leg alone
            self._spec = [torch.empty((1, FEAT_C, engine.SPEC_W), dtype=torch.float32, device=dev) if self.side.has_spectrum else None
                          for _ in range(2)]
            self._dc = ([torch.empty((1, engine.DELTA_CACHE_ELEMS), dtype=torch.float32, device=dev) for _ in range(2)]
                        if with_delta_cache and engine.has_delta_cache else None)
            self._ready = [torch.cuda.Event(), torch.cuda.Event()]
            self._released = [None, None]      # recorded on the consumer's stream behind the last reader of a slot's contents
            self._has_dc = [False, False]      # did the slot's last submit compute the Delta cache row?
        self._submitted = 0
        self._taken = 0
        self._last = None                      # slot handed out by the latest take(), not yet released

    def _release_last(self) -> None:
        """The consumer has enqueued its readers of the slot last handed out by now (contract above): an event behind them on the
        current stream is what the next overwrite of that slot waits for."""
        if self._last is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.main.device))
            self._released[self._last] = ev
            self._last = None

    def submit(self, image: torch.Tensor, wait_current: bool = True, with_delta: bool = True) -> None:
        """Enqueue leg + spectrum of `image` (1, in_h, in_w, in_c) on the side stream; at most two queries may be in flight.
        `wait_current=False`: the image was produced on `self.stream` itself (e.g. its host-to-device copy was issued there), so the
        side stream need not wait for the work already enqueued on the caller's stream -- except for the readers of the slot it is
        about to overwrite, which it always waits for.  `with_delta=False`: skip this query's Delta cache row even if the object was
        built `with_delta_cache` (a sharded `Infer` whose rank does not own the frame); `take_all` then returns None for it."""
        if self._submitted - self._taken >= 2:
            raise _lib.OvnError("QueryAhead.submit: two queries are already in flight, take() one first")
        self._release_last()
        slot = self._submitted & 1
        if self.side.leg_precision != self.main.leg_precision:       # follow the main engine's arithmetic (same bits as engine.leg)
            self.side.set_leg_precision(self.main.leg_precision)
        if self.side.head_precision != self.main.head_precision:
            self.side.set_head_precision(self.main.head_precision)
        if self.side.head_width_split != self.main.head_width_split:
            self.side.set_head_width_split(self.main.head_width_split)
        if self.side.projection_trig != self.main.projection_trig:
            self.side.set_projection_trig(self.main.projection_trig)
        if self.side.corr_normalization != self.main.corr_normalization:
            self.side.set_corr_normalization(self.main.corr_normalization)
        if wait_current:
            self.stream.wait_stream(torch.cuda.current_stream(self.main.device))   # the image belongs to the caller's stream
        if self._released[slot] is not None:
            self.stream.wait_event(self._released[slot])     # the heads that read this slot two queries ago are done with it
        with torch.cuda.stream(self.stream):
            self.side.leg(image, out=self._fv[slot])
            if self._spec[slot] is not None:
                self.side.spectrum(self._fv[slot], out=self._spec[slot])
            self._has_dc[slot] = self._dc is not None and bool(with_delta)
            if self._has_dc[slot]:
                self.side.delta_cache(self._fv[slot], out=self._dc[slot])
            self._ready[slot].record(self.stream)
        image.record_stream(self.stream)
        self._submitted += 1

    def take(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(feature volume (1, W, 128), spectrum or None at W != 360) of the oldest submitted query; the CURRENT stream waits for them, the host does
        not.  Readers of the pair must be enqueued on the current stream before the next submit() / take() call (class docstring)."""
        if self._taken >= self._submitted:
            raise _lib.OvnError("QueryAhead.take: nothing submitted")
        self._release_last()
        slot = self._taken & 1
        cur = torch.cuda.current_stream(self.main.device)
        cur.wait_event(self._ready[slot])
        self._taken += 1
        self._last = slot
        self._last_taken = slot
        return self._fv[slot], self._spec[slot]

    def take_all(self):
        """take() plus the Delta cache row (None unless built with `with_delta_cache` on a head geometry that has one)."""
        fv, spec = self.take()
        return fv, spec, (self._dc[self._last_taken] if self._has_dc[self._last_taken] else None)

    def close(self) -> None:
        self.stream.synchronize()
        self.side.close()


def segment_table(seg_offsets, query_idx, n_queries: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    """Host check of a segmented batch's table (`heads_segments`, `top_k_segments`): (offsets int64 (B + 1), query_idx int32 (B)).
    Raises ValueError for offsets that do not start at 0 or decrease, IndexError for a query index outside [0, n_queries).  No GPU."""
    def host(a):
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    o = host(seg_offsets).reshape(-1)
    if o.size == 0 or (o.size and not np.issubdtype(o.dtype, np.integer)):
        raise ValueError("seg_offsets must be B + 1 >= 1 integers")
    o = np.ascontiguousarray(o, dtype=np.int64)
    if o[0] != 0:
        raise ValueError("seg_offsets[0] must be 0, got %d" % int(o[0]))
    if np.any(np.diff(o) < 0):
        raise ValueError("seg_offsets must be non-decreasing")
    if int(o[-1]) >= 1 << 31:
        raise ValueError("more than 2^31 - 1 pairs in one batch")
    if query_idx is None:
        return o, np.zeros(0, np.int32)
    q = host(query_idx).reshape(-1)
    if q.size != o.size - 1:
        raise ValueError("query_idx has %d entries for %d segments" % (q.size, o.size - 1))
    if q.size and not np.issubdtype(q.dtype, np.integer):
        raise IndexError("query_idx holds non-integer values")
    q = q.astype(np.int64)
    if q.size and (int(q.min()) < 0 or (n_queries is not None and int(q.max()) >= n_queries)):
        raise IndexError("query index out of range: [%d, %d] not within [0, %s)" % (int(q.min()), int(q.max()), n_queries))
    return o, np.ascontiguousarray(q, dtype=np.int32)


def check_top_k(k) -> int:
    """k of the top-k calls: an integer in 1..OVN_TOP_K_MAX (1024), else ValueError."""
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError("k must be in 1..1024, got %d" % k)
    return k


def decode_match(record) -> Optional[Tuple[int, float, int]]:
    """(candidate id, overlap, yaw) from a best-match record, or None when nothing exceeded the threshold."""
    import numpy as np

    r = np.asarray(record.cpu() if hasattr(record, "cpu") else record, dtype=np.int32).reshape(4)
    if r[3] == 0 or r[0] < 0:
        return None
    return int(r[0]), float(r[1:2].view(np.float32)[0]), int(r[2])


def decode_top_k(records) -> List[Tuple[int, float, int, bool]]:
    """[(candidate id, overlap, yaw, overlap > threshold)] from top-k records, best first; the {-1, 0, 0, 0} rows are dropped."""
    r = np.asarray(records.cpu() if hasattr(records, "cpu") else records, dtype=np.int32).reshape(-1, 4)
    ov = r[:, 1].copy().view(np.float32)
    return [(int(r[i, 0]), float(ov[i]), int(r[i, 2]), bool(r[i, 3] > 0)) for i in range(len(r)) if r[i, 0] >= 0]
