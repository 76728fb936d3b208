"""CPU: what the host wrapper hands to the library, call by call, held against a recorded sequence.

An `OvnEngine` is made with `OvnEngine.__new__`, given the plain attributes `__init__` would set, the CPU as its device and a recorder
in place of the library.  Only `_dev` and `_stream` are patched.  Every public method that reaches a native call is driven once per
native route with the smallest valid CPU tensors; the recorder holds each call against `_lib.SIGNATURES` (argument count, and every
argument accepted by its argtype's `from_param`, as ctypes would at the real call) and notes it down.  The sequence must equal
tests/golden/engine_calls.json.  A wrapper that passes the wrong number, order or type of arguments fails here, without a GPU.

`python -m tests.test_engine_calls_host --record` writes the golden file from the tree it runs in."""
import contextlib
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from overlapnet_amd import _lib
from overlapnet_amd import engine as E
from overlapnet_amd import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_calls.json")
MAX_EXEMPT = 6
# a method name exempts the method; "method(route)" exempts one route of a method that is covered otherwise
EXEMPT = {
    "load_weights": "ends in torch.cuda.synchronize(device), which needs a HIP device; tests/test_gpu_api.py loads weights",
    "best_match(host=True)": "writes its record into pinned host memory, which torch allocates through the HIP runtime only",
}
# context queries that a method may make before it has looked at its tensors; a refused call reaches nothing else
SIZE_QUERIES = {"ovn_head_param_sizes", "ovn_leg_layer_count", "ovn_leg_param_sizes", "ovn_leg_activation_sizes",
                "ovn_pose_graph_workspace_bytes", "ovn_pose_graph_loops_bytes", "ovn_pose_graph_loops_layout",
                "ovn_pose_graph_marginals_bytes"}
IN_H, IN_W, IN_C, FW = 32, 200, 2, 360
HANDLE, STREAM = 0x1000, 0x2000


def _is_pointer(argtype):
    return argtype in (C.c_void_p, C.c_char_p) or hasattr(argtype, "contents")


class Recorder:
    """Stands in for the CDLL: every ovn_* attribute checks its arguments against SIGNATURES, notes the call and returns 0."""

    def __init__(self):
        self.calls = []
        self.names = {HANDLE: "handle", STREAM: "stream"}      # address -> the name a pointer is noted under
        self.keep = []                                         # the named tensors stay alive, so no address is used twice
        layers = W.leg_layers(IN_C, {})
        shapes = W.expected_shapes(IN_C, {}, FW)
        acts, h, w = [], IN_H, IN_W
        for l in layers:
            h, w = (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1
            acts.append(h * w * l.cout)
        self.fills = {      # name -> (index of the output argument, what the library writes there)
            "ovn_head_param_sizes": (1, [int(np.prod(shapes[k])) for k in E.OvnEngine.HEAD_PARAMS]),
            "ovn_leg_layer_count": (1, [len(layers)]),
            "ovn_leg_param_sizes": (1, [v for l in layers for v in (l.kh * l.kw * l.cin * l.cout, l.cout)]),
            "ovn_leg_activation_sizes": (1, acts),
            "ovn_get_corr_normalization": (1, [2]),
            "ovn_get_head_width_split": (1, [1]),
        }

    def name(self, **tensors):
        for k, t in tensors.items():
            if isinstance(t, torch.Tensor) and t.numel():
                self.names[t.data_ptr()] = k
                self.keep.append(t)

    @staticmethod
    def _loops_layout(n, nl):
        sp = 6 * nl
        sizes = [36 * n, 36 * nl, 36 * nl, 4 * nl, sp * sp, sp * sp]
        offs = [int(sum(sizes[:i])) for i in range(6)]
        return [6, sp] + offs, int(sum(sizes))

    def _result(self, name, args):
        if name == "ovn_pose_graph_workspace_bytes":
            return 8 * (64 + 12 * args[0] + 6 * args[1])
        if name == "ovn_pose_graph_loops_bytes":
            return 8 * self._loops_layout(args[0], args[1])[1] if 1 <= args[1] <= 256 else 0
        if name == "ovn_pose_graph_marginals_bytes":
            return 8 * (64 + args[0] + 36 * args[2])
        if name == "ovn_workspace_bytes":
            return 4096
        if name == "ovn_pose_graph_loops_layout":
            for i, v in enumerate(self._loops_layout(args[0], args[1])[0]):
                args[2][i] = v
        if name in self.fills:
            i, values = self.fills[name]
            target = args[i]._obj if hasattr(args[i], "_obj") else args[i]
            if isinstance(target, C.Array):
                for j, v in enumerate(values):
                    target[j] = v
            else:
                target.value = values[0]
        return 0

    def _note(self, argtype, a):
        if not _is_pointer(argtype):
            return float(a) if argtype in (C.c_float, C.c_double) else int(a)
        if a is None:
            return "null"
        if isinstance(a, C.Array):                 # a small host array: its contents are part of the call
            return ["host", [v for v in a]]
        if isinstance(a, bytes):
            return ["bytes", a.decode()]
        addr = a if isinstance(a, int) else getattr(a, "value", -1)
        if addr is None:
            return "null"
        return self.names.get(addr, "ptr")

    def __getattr__(self, name):
        if not name.startswith("ovn_"):
            raise AttributeError(name)
        res, argtypes = _lib.SIGNATURES[name]

        def fn(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, the wrapper passes %d" % (name, len(argtypes), len(args))
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as exc:
                    raise AssertionError("%s: argument %d (%r) is no %s: %s" % (name, i, a, t.__name__, exc))
            self.calls.append([name, [self._note(t, a) for t, a in zip(argtypes, args)]])
            return self._result(name, args)
        return fn


def make_engine():
    e = E.OvnEngine.__new__(E.OvnEngine)
    rec = Recorder()
    e.lib = rec
    e.device_index = 0
    e.device = torch.device("cpu")
    e.in_h, e.in_w, e.in_c = IN_H, IN_W, IN_C
    e._h = C.c_void_p(HANDLE)
    e.feat_w = FW
    e._leg_ready = e._head_ready = True
    e.head_precision = e.leg_precision = "f16x3"
    e.head_width_split = False
    e.projection_trig = "numpy_avx512"
    e.head_compaction = True
    e.negate_diffs = False
    e.conv1size = 15
    e._leg_cfg = {}
    e.check_device_indices = False
    e._render_tables = {}
    e._dev = lambda: contextlib.nullcontext()
    e._stream = lambda: C.c_void_p(STREAM)
    return e, rec


def _summary(v):
    """What a call returned, without the numbers: types, dtypes and shapes."""
    if isinstance(v, torch.Tensor):
        return [str(v.dtype), list(v.shape)]
    if isinstance(v, np.ndarray):
        return ["ndarray", str(v.dtype), list(v.shape)]
    if isinstance(v, dict):
        return {k: _summary(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_summary(x) for x in v]
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    return type(v).__name__


class _Mesh:
    """What render_scans asks of a mesh.TriangleMesh."""
    n_vertices, n_triangles = 4, 2

    def __init__(self):
        self.d = {"vertices": torch.rand(4, 3), "triangles": torch.zeros((2, 3), dtype=torch.int32),
                  "nodes": torch.rand(3, 8), "order": torch.zeros(2, dtype=torch.int32), "leaves": 2}

    def device(self, engine, with_bvh=True):
        return self.d


class Driver:
    """Runs the table of calls below on one fake engine.  `steps` keeps (label, method, kwargs) for the refusal test."""

    def __init__(self):
        self.e, self.rec = make_engine()
        self.steps = []
        self.covered = set()

    def call(self, label, method, **kw):
        for k, v in kw.items():
            self.rec.name(**({k: v} if not isinstance(v, dict) else {"%s[%s]" % (k, n): t for n, t in v.items()}))
        self.rec.calls.append(["call", label])
        self.steps.append((label, method, kw))
        self.covered.add(method)
        r = self.invoke(method, kw)
        self.rec.calls.append(["return", _summary(r)])
        return r

    def invoke(self, method, kw):
        if isinstance(inspect.getattr_static(E.OvnEngine, method), property):
            return getattr(self.e, method)
        return getattr(self.e, method)(**kw)


def f32(*shape):
    return torch.rand(*shape, dtype=torch.float32)


def f64(*shape):
    return torch.rand(*shape, dtype=torch.float64)


def i32(*values):
    return torch.tensor(values, dtype=torch.int32)


def drive():
    d = Driver()
    e, call = d.e, d.call
    dc = e.DELTA_CACHE_ELEMS

    # -- leg, heads ------------------------------------------------------------------------------------------------------
    images = f32(2, IN_H, IN_W, IN_C)
    call("leg", "leg", images=images)
    call("leg out=", "leg", images=images, out=f32(2, FW, 128))
    fl, fr = f32(3, FW, 128), f32(2, FW, 128)
    sl, sr = f32(3, 128, 368), f32(2, 128, 368)
    dl = f32(3, dc)
    call("heads", "heads", feats_l=fl, feats_r=fr)
    call("heads indexed, logit, corr", "heads", feats_l=fl, feats_r=fr, lidx=[2, 0], ridx=[1, 1], want_logit=True, want_corr=True)
    call("heads spectra", "heads", feats_l=fl, feats_r=fr, spec_l=sl, spec_r=sr, want_corr=True)
    call("heads spectra, delta cache", "heads", feats_l=fl, feats_r=fr, spec_l=sl, spec_r=sr, dcache_l=dl, lidx=[1], want_logit=True)
    seg = dict(feats_pool=fl, feats_q=fr, cand_idx=[0, 2, 1], query_idx=[1, 0], seg_offsets=[0, 2, 3])
    call("heads_segments", "heads_segments", **seg)
    call("heads_segments spectra, delta cache", "heads_segments", spec_pool=sl, spec_q=sr, dcache_pool=dl, want_logit=True,
         want_corr=True, **seg)
    call("corr_head", "corr_head", feats_l=fl, feats_r=fr)
    call("corr_head corr", "corr_head", feats_l=fl, feats_r=fr, lidx=[0, 1], ridx=[1, 0], want_corr=True)
    call("delta_cache", "delta_cache", feats=fl)
    call("delta_cache out=", "delta_cache", feats=fl, out=f32(3, dc))
    call("spectrum", "spectrum", feats=fl)
    call("spectrum out=", "spectrum", feats=fl, out=f32(3, 128, 368))
    call("corr_head_spectral", "corr_head_spectral", spec_l=sl, spec_r=sr)
    call("corr_head_spectral corr", "corr_head_spectral", spec_l=sl, spec_r=sr, lidx=[0, 1], ridx=[1, 0], want_corr=True)
    call("debug_head_activations", "debug_head_activations", n=2)

    # -- training --------------------------------------------------------------------------------------------------------
    call("head_param_sizes", "head_param_sizes")
    sizes = d.rec.fills["ovn_head_param_sizes"][1]
    call("set_head_weights", "set_head_weights", params=[f32(s) for s in sizes])
    call("delta_head_grad", "delta_head_grad", feats_l=fl, feats_r=fr, targets=[0.5, 0.25])
    call("delta_head_grad mse, activations", "delta_head_grad", feats_l=fl, feats_r=fr, targets=f32(2), lidx=[0, 2], ridx=[1, 0],
         loss="mse", scale=2.0, want_activations=True)
    call("heads_feature_grad", "heads_feature_grad", feats_l=fl, feats_r=fr, targets=[0.5, 0.75])
    call("heads_feature_grad yaw, head grads", "heads_feature_grad", feats_l=fl, feats_r=fr, targets=f32(2), yaw_bins=[3, 400],
         lidx=[0, 2], ridx=[1, 0], loss="mse", want_head_grads=True, want_corr=False)
    call("leg_param_shapes", "leg_param_shapes")
    call("leg_activation_shapes", "leg_activation_shapes")
    acts = call("leg_forward_train", "leg_forward_train", images=images)
    call("leg_backward", "leg_backward", images=images, acts=acts, dfeat=f32(2, FW, 128), slice_scans=1)
    pshapes = e.leg_param_shapes()
    call("set_leg_weights list", "set_leg_weights", params=[f32(*s) for s in pshapes])
    call("set_leg_weights one layer", "set_leg_weights", params={"s_conv2/kernel": f32(*pshapes[2]), "s_conv2/bias": f32(*pshapes[3])})
    grads = f32(2, 8)
    call("grad_reduce_adagrad reduce", "grad_reduce_adagrad", grads=grads, rank_weights=[0.5, 0.5], count=6)
    call("grad_reduce_adagrad update", "grad_reduce_adagrad", grads=grads, rank_weights=[0.25, 0.75], params=f32(7), accum=f32(7), lr=0.01,
         want_grad=True)
    x = f32(1, 8, 20, IN_C)
    call("debug_conv", "debug_conv", layer=0, x=x)
    o = f32(1, 2, 3, 16)
    call("debug_conv_grad", "debug_conv_grad", layer=0, x=x, out=o, dout=f32(1, 2, 3, 16))
    call("debug_conv_grad din", "debug_conv_grad", layer=0, x=x, out=o, dout=f32(1, 2, 3, 16), want=("din",))

    # -- ground truth ----------------------------------------------------------------------------------------------------
    points = f32(10, 4)
    offsets = torch.tensor([0, 4, 10], dtype=torch.int64)
    poses2, inv2 = f64(2, 4, 4), f64(2, 4, 4)
    call("gt_range_images", "gt_range_images", points=points, offsets=offsets, max_points=6, proj_h=4, proj_w=8)
    call("gt_range_images poses", "gt_range_images", points=points, offsets=offsets, max_points=6, ref_poses=poses2, inv_cur_pose=f64(4, 4),
         proj_h=4, proj_w=8)
    rr = f32(2, 4, 8)
    call("gt_overlap_counts", "gt_overlap_counts", ref_ranges=rr, cur_range=f32(4, 8))
    call("gt_pair_counts", "gt_pair_counts", points=points, offsets=offsets, poses=poses2, inv_poses=inv2, cur_ranges=rr)
    call("gt_pair_counts lists", "gt_pair_counts", points=points, offsets=offsets, poses=poses2, inv_poses=inv2, cur_ranges=rr,
         frame_idx=i32(1, 0, 1), ref_idx=i32(0, 0))

    # -- decisions -------------------------------------------------------------------------------------------------------
    ov, yw, ids = f32(6), torch.arange(6, dtype=torch.int32), torch.arange(6, dtype=torch.int32) + 10
    call("best_match", "best_match", overlap=ov)
    call("best_match yaw, ids", "best_match", overlap=ov, yaw=yw, threshold=0.5, ids=ids, index_offset=3)
    call("top_k", "top_k", overlap=ov, k=2)
    call("top_k yaw, ids, out=", "top_k", overlap=ov, yaw=yw, k=3, ids=ids, index_offset=5, out=torch.zeros((3, 4), dtype=torch.int32))
    call("top_k_segments", "top_k_segments", overlap=ov, seg_offsets=[0, 4, 6], k=2)
    call("top_k_segments yaw, ids, out=", "top_k_segments", overlap=ov, seg_offsets=[0, 4, 6], yaw=yw, k=2, ids=ids,
         out=torch.zeros((2, 2, 4), dtype=torch.int32))

    # -- projection, rendering, TSDF -------------------------------------------------------------------------------------
    proj = dict(points=points, offsets=offsets, max_points=6, proj_h=4, proj_w=8)
    call("project", "project", **proj)
    call("project all outputs", "project", want=("range", "vertex", "intensity", "idx", "normal", "no such output"), **proj)
    call("project stacked", "project", want=("range",), stacked_flags=(True, True, False), **proj)
    call("project stacked none", "project", want=(), stacked_flags=(False, False, False), **proj)
    call("project stacked_out=", "project", want=(), stacked_flags=(True, False, True), stacked_out=f32(2, 4, 8, 2), **proj)
    probs = f32(10, 3)
    call("project semantic", "project", probs=probs, n_classes=3, want=("range", "semantic", "sem_idx"), **proj)
    call("project semantic, n_points, stacked", "project", probs=probs, n_classes=3, n_points=10, want=("normal",),
         stacked_flags=(True, False, True, True), **proj)
    call("project semantic stacked_out=", "project", probs=probs, n_classes=3, n_points=10, want=("vertex", "intensity", "idx"),
         stacked_flags=(False, True, True, False), stacked_out=f32(2, 4, 8, 6), **proj)
    call("normals", "normals", rng=rr, vtx=f32(2, 4, 8, 4))
    call("projection_angles", "projection_angles", points=points, proj_h=4, proj_w=8)
    mesh = _Mesh()
    d.rec.name(**{"mesh[%s]" % k: v for k, v in mesh.d.items()})
    view = dict(proj_h=4, proj_w=8)
    call("render_scans", "render_scans", mesh=mesh, poses=np.tile(np.eye(4), (2, 1, 1)), **view)
    call("render_scans exhaustive, all outputs", "render_scans", mesh=mesh, poses=poses2, want=("range", "tri_id", "vertex", "normal"),
         exhaustive=True, **view)
    call("render_scans stacked", "render_scans", mesh=mesh, poses=poses2, want=(), stacked_flags=(True, True), **view)
    call("render_scans stacked none", "render_scans", mesh=mesh, poses=poses2, want=("range",), stacked_flags=(False,), **view)
    call("render_scans stacked_out=", "render_scans", mesh=mesh, poses=poses2, want=(), stacked_flags=(True, False, False, False),
         stacked_out=f32(2, 4, 8, 1), **view)
    tsdf, weight = f32(9, 10, 17), f32(9, 10, 17)
    vol = dict(tsdf=tsdf, weight=weight, origin=(-1.0, 0.5, 2.0), voxel=0.25)
    win = dict(vol, base=(3, -4, 5))
    for label, v in (("dense", vol), ("window", win)):
        call("tsdf_integrate " + label, "tsdf_integrate", trunc=1.0, max_weight=64.0, range_images=rr, poses=poses2, **v)
        call("tsdf_raycast " + label, "tsdf_raycast", poses=poses2, **view, **v)
        call("tsdf_raycast %s, bricks, step, stacked" % label, "tsdf_raycast", poses=np.tile(np.eye(4), (2, 1, 1)), step=0.1,
             bricks=torch.zeros((2, 2, 3), dtype=torch.uint8), want=("vertex",), stacked_flags=(True, True), **view, **v)
        call("tsdf_raycast %s, stacked none" % label, "tsdf_raycast", poses=poses2, want=(), stacked_flags=(False, False), **view, **v)
        call("tsdf_raycast %s, out=, stacked_out=" % label, "tsdf_raycast", poses=poses2, want=("range",),
             out={"normal": f32(2, 4, 8, 3), "range": f32(2, 4, 8)}, stacked_flags=(False, True), stacked_out=f32(2, 4, 8, 3), **view, **v)
    call("tsdf_triangles dense, count then write", "tsdf_triangles", **vol)
    call("tsdf_triangles dense, capacity", "tsdf_triangles", capacity=4, min_weight=2.0, **vol)
    call("tsdf_triangles dense, out=", "tsdf_triangles", out=f32(5, 3, 3), **vol)
    box = ((3, -4, 5), (10, 2, 9))
    call("tsdf_triangles window, count only", "tsdf_triangles", capacity=0, box=box, **win)
    call("tsdf_triangles window, capacity", "tsdf_triangles", capacity=4, box=box, **win)
    call("tsdf_bricks", "tsdf_bricks", weight=weight, min_weight=2.0)
    call("tsdf_bricks out=", "tsdf_bricks", weight=weight, out=torch.zeros((2, 2, 3), dtype=torch.uint8))
    call("tsdf_window_shift", "tsdf_window_shift", tsdf=tsdf, weight=weight, old_base=(3, -4, 5), new_base=np.array([4, -4, 2]))
    call("icp_register", "icp_register", vertex=f32(2, 4, 8, 4), normal=f32(2, 4, 8, 3), rng=rr, src_idx=i32(0, 1, 1), tgt_idx=i32(1, 0, 1),
         init_pose=f64(3, 4, 4))
    call("icp_register system", "icp_register", vertex=f32(2, 4, 8, 4), normal=f32(2, 4, 8, 3), rng=rr, src_idx=i32(0, 1), tgt_idx=i32(1, 0),
         init_pose=f64(2, 4, 4), iterations=5, want_system=True)

    # -- Monte Carlo localization ----------------------------------------------------------------------------------------
    parts = f32(5, 4)
    grid = dict(cell_frame=torch.zeros(6, dtype=torch.int32), origin=(-1.0, 2.0), resolution=0.5, nx=3, ny=2, n_frames=4)
    mcl = dict(particles=parts, odom=(0.1, 0.2, 0.3), sigma=(0.01, 0.02, 0.03), seed=7, step=2 ** 64 + 3, **grid)
    call("mcl_predict", "mcl_predict", **mcl)
    pf, fs, flist = torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    call("mcl_predict buffers", "mcl_predict", particle_frame=pf, frame_slot=fs, frame_list=flist, record=torch.zeros(4, dtype=torch.int32),
         **mcl)
    upd = dict(particles=parts, particle_frame=pf, frame_slot=fs, frame_yaw=f32(4), sigma_yaw=0.2, eps_yaw=0.01, overlap_min=0.3)
    call("mcl_update", "mcl_update", overlap=f32(3), yaw=i32(1, 2, 3), **upd)
    call("mcl_update nothing seen, spread", "mcl_update", overlap=None, yaw=None, estimate=f64(8), want_spread=True, **upd)
    call("mcl_resample", "mcl_resample", particles=parts, seed=-1, step=4)
    call("mcl_resample buffers", "mcl_resample", particles=parts, seed=1, step=4, n_out=3, out=f32(3, 4),
         ancestors=torch.zeros(3, dtype=torch.int32), record=torch.zeros(4, dtype=torch.int32))

    # -- settings --------------------------------------------------------------------------------------------------------
    call("set_head_pipeline", "set_head_pipeline", chunk_pairs=512, sub_chunk_pairs=64, streams=2, yaw_on_side_stream=True)
    call("head_pipeline", "head_pipeline")
    call("set_head_precision", "set_head_precision", mode="bf16x3")
    call("set_head_width_split", "set_head_width_split", on=True)
    call("set_corr_normalization", "set_corr_normalization", mode="scaling")
    call("corr_normalization", "corr_normalization")
    call("set_head_compaction", "set_head_compaction", on=False)
    call("head_walk_stats", "head_walk_stats")
    call("set_projection_trig", "set_projection_trig", mode="rounded")
    call("set_leg_precision", "set_leg_precision", mode="f32")
    call("profile_begin", "profile_begin")
    call("profile_end", "profile_end")
    call("selftest", "selftest")
    call("workspace_bytes", "workspace_bytes")

    # -- pose graph ------------------------------------------------------------------------------------------------------
    n, nl = 4, 2
    ne = n - 1 + nl
    g = dict(poses=f64(n, 4, 4), fixed=torch.zeros(n, dtype=torch.uint8), edge_ij=torch.zeros((ne, 2), dtype=torch.int32), meas=f64(ne, 4, 4),
             info=f64(ne, 6, 6), node_ptr=torch.zeros(n + 1, dtype=torch.int32), node_edge=torch.zeros(2 * ne, dtype=torch.int32))
    topo = {k: g[k] for k in ("fixed", "edge_ij", "node_ptr", "node_edge")}
    plain = call("pose_graph_buffers", "pose_graph_buffers", n_nodes=n, n_edges=ne)
    chain = call("pose_graph_buffers chain", "pose_graph_buffers", n_nodes=n, n_edges=ne, chain=True)
    loops = call("pose_graph_buffers loops", "pose_graph_buffers", n_nodes=n, n_edges=ne, loops=nl)
    call("pose_graph_linearize", "pose_graph_linearize", huber=1.5, buf=plain, **g)
    call("pose_graph_linearize chain, residuals only, record=", "pose_graph_linearize", huber=1.5, buf=chain, jacobians=False, record=f64(16), **g)
    call("pose_graph_linearize loops", "pose_graph_linearize", huber=1.5, buf=loops, **g)
    call("pose_graph_solve jacobi", "pose_graph_solve", buf=plain, **topo)
    call("pose_graph_solve chain", "pose_graph_solve", buf=chain, preconditioner="chain", lam=0.5, rtol=1e-6, first_iteration=3, iterations=8,
         **topo)
    call("pose_graph_solve loops", "pose_graph_solve", buf=loops, preconditioner="loops", iterations=4, **topo)
    call("pose_graph_loops_prepare", "pose_graph_loops_prepare", poses=g["poses"], edge_ij=g["edge_ij"], info=g["info"], buf=loops)
    call("pose_graph_loops_prepare record=, stages", "pose_graph_loops_prepare", poses=g["poses"], edge_ij=g["edge_ij"], info=g["info"],
         buf=loops, record=f64(16), stages=3)
    call("pose_graph_loops_views", "pose_graph_loops_views", buf=loops, n_nodes=n, n_loops=nl)
    vec = f64(n, 6)
    call("pose_graph_precondition jacobi", "pose_graph_precondition", vec=vec, buf=plain)
    call("pose_graph_precondition chain, out=", "pose_graph_precondition", vec=vec, buf=chain, preconditioner=1, lam=0.25, out=f64(n, 6))
    call("pose_graph_precondition loops", "pose_graph_precondition", vec=vec, buf=loops, preconditioner="loops", node_ptr=g["node_ptr"],
         node_edge=g["node_edge"])
    call("pose_graph_marginals_bytes", "pose_graph_marginals_bytes", n_nodes=n, n_loops=nl, n_query=2)
    call("pose_graph_marginals chain", "pose_graph_marginals", poses=g["poses"], buf=chain, node_ids=i32(0, 3), n_loops=0)
    call("pose_graph_marginals loops, local, buffers", "pose_graph_marginals", poses=g["poses"], buf=loops, node_ids=i32(1, 2, 3), n_loops=nl,
         frame="local", cov=f64(3, 6, 6), ws=f64(400), record=f64(16))
    call("pose_graph_retract", "pose_graph_retract", poses=g["poses"], fixed=g["fixed"], buf=plain)
    call("pose_graph_retract out=, record=", "pose_graph_retract", poses=g["poses"], fixed=g["fixed"], buf=plain, out=f64(n, 4, 4), record=f64(16))
    call("close", "close")
    return d


# For each method with tensor arguments: (label of a step above, argument, corruptions the wrapper refuses with an OvnError).
# "dtype": another dtype; "strided": same shape and dtype, not contiguous; "shape": one element more, flat.
REFUSED = [
    ("leg", "images", "dtype strided shape"), ("leg_forward_train", "images", "dtype strided shape"),
    ("leg_backward", "dfeat", "dtype strided shape"), ("leg_backward", "images", "dtype strided shape"),
    ("heads", "feats_l", "dtype strided shape"), ("heads spectra", "spec_r", "dtype strided shape"),
    ("heads spectra, delta cache", "dcache_l", "dtype strided shape"),
    ("heads_segments", "feats_q", "dtype strided shape"), ("heads_segments spectra, delta cache", "spec_pool", "dtype strided shape"),
    ("heads_segments spectra, delta cache", "dcache_pool", "dtype strided shape"),
    ("corr_head", "feats_r", "dtype strided shape"), ("delta_cache", "feats", "dtype strided shape"),
    ("spectrum", "feats", "dtype strided shape"), ("corr_head_spectral", "spec_l", "dtype strided shape"),
    ("delta_head_grad", "feats_l", "dtype strided shape"), ("heads_feature_grad", "feats_r", "dtype strided shape"),
    ("grad_reduce_adagrad reduce", "grads", "dtype strided shape"), ("grad_reduce_adagrad update", "accum", "dtype strided shape"),
    ("debug_conv_grad", "dout", "dtype strided shape"),
    ("gt_range_images poses", "ref_poses", "dtype strided shape"), ("gt_range_images", "offsets", "dtype strided"),
    ("gt_overlap_counts", "cur_range", "dtype strided shape"), ("gt_pair_counts", "inv_poses", "dtype strided shape"),
    ("gt_pair_counts lists", "frame_idx", "dtype strided"),
    ("best_match yaw, ids", "yaw", "dtype strided shape"), ("top_k yaw, ids, out=", "ids", "dtype strided shape"),
    ("top_k yaw, ids, out=", "out", "dtype strided shape"), ("top_k_segments yaw, ids, out=", "overlap", "dtype strided shape"),
    ("top_k_segments yaw, ids, out=", "out", "dtype strided shape"),
    ("project", "points", "dtype strided"), ("project", "offsets", "dtype"), ("project stacked_out=", "stacked_out", "dtype strided shape"),
    ("project semantic", "probs", "dtype strided shape"), ("project semantic stacked_out=", "stacked_out", "dtype strided shape"),
    ("normals", "vtx", "dtype strided shape"), ("projection_angles", "points", "dtype strided shape"),
    ("render_scans stacked_out=", "stacked_out", "dtype strided shape"),
    ("tsdf_integrate dense", "range_images", "dtype strided shape"), ("tsdf_integrate window", "weight", "dtype strided shape"),
    ("tsdf_triangles dense, out=", "out", "dtype strided shape"), ("tsdf_triangles window, capacity", "tsdf", "dtype strided shape"),
    ("tsdf_bricks", "weight", "dtype strided shape"), ("tsdf_bricks out=", "out", "dtype strided shape"),
    ("tsdf_raycast dense, bricks, step, stacked", "bricks", "dtype strided shape"),
    ("tsdf_raycast window, out=, stacked_out=", "stacked_out", "dtype strided shape"),
    ("tsdf_raycast dense", "tsdf", "dtype strided shape"), ("tsdf_window_shift", "weight", "dtype strided shape"),
    ("icp_register", "normal", "dtype strided shape"), ("icp_register", "init_pose", "dtype strided shape"),
    ("mcl_predict buffers", "particles", "dtype strided shape"), ("mcl_predict buffers", "record", "dtype strided shape"),
    ("mcl_update", "frame_yaw", "dtype strided shape"), ("mcl_update", "yaw", "dtype strided shape"),
    ("mcl_resample buffers", "ancestors", "dtype strided shape"), ("mcl_resample buffers", "out", "dtype strided shape"),
    ("pose_graph_linearize", "meas", "dtype strided shape"), ("pose_graph_linearize", "fixed", "dtype strided shape"),
    ("pose_graph_loops_prepare", "info", "dtype strided shape"),
    ("pose_graph_precondition chain, out=", "out", "dtype strided shape"), ("pose_graph_precondition loops", "node_ptr", "dtype strided shape"),
    ("pose_graph_marginals loops, local, buffers", "cov", "dtype strided shape"),
    ("pose_graph_marginals chain", "node_ids", "dtype strided"), ("pose_graph_retract out=, record=", "out", "dtype strided shape"),
    ("set_head_weights", "params", "dtype shape"), ("set_leg_weights list", "params", "dtype shape"),
]
# methods with tensor arguments that the wrapper hands on as they are (the library checks what it can)
UNCHECKED = {"debug_conv": "takes x.contiguous() and leaves the rest to the library",
             "pose_graph_solve": "reads the buffers of pose_graph_linearize, which checked them",
             "pose_graph_loops_views": "only slices buf['loops'], which _pg_loops checks against the layout"}


def _corrupt(t, kind):
    if isinstance(t, (list, tuple)):                      # a list of tensors: spoil the first one
        return [_corrupt(t[0], kind)] + list(t[1:])
    if kind == "dtype":
        return t.to(torch.int16) if not t.is_floating_point() else t.to(torch.float64 if t.dtype == torch.float32 else torch.float32)
    if kind == "strided":
        s = torch.stack([t, t], dim=-1)[..., 0]
        assert not s.is_contiguous() and s.shape == t.shape
        return s
    flat = t.reshape(-1)
    return torch.cat([flat, flat[:1]])


@pytest.fixture(scope="module")
def driven():
    torch.manual_seed(0)
    return drive()


def _library_callers():
    """The public methods (and properties) of OvnEngine whose own source names an ovn_* function outside its docstring."""
    names = set()
    for name, member in vars(E.OvnEngine).items():
        if name.startswith("_"):
            continue
        fn = member.fget if isinstance(member, property) else member
        if not inspect.isfunction(fn):
            continue
        src = inspect.getsource(fn)
        if fn.__doc__:
            src = src.replace(fn.__doc__, "")
        if re.search(r"\bovn_\w+", src):
            names.add(name)
    return names


def test_every_library_caller_is_driven_or_exempt(driven):
    callers = _library_callers()
    assert len(callers) >= 60
    exempt_methods = {k for k in EXEMPT if "(" not in k}
    assert driven.covered | exempt_methods == callers, (sorted(callers - driven.covered - exempt_methods),
                                                         sorted((driven.covered | exempt_methods) - callers))
    assert not driven.covered & exempt_methods
    for route in (k for k in EXEMPT if "(" in k):
        assert route.split("(")[0] in driven.covered, route


def test_exemptions_are_few_and_reasoned():
    assert len(EXEMPT) <= MAX_EXEMPT
    assert "best_match(host=True)" in EXEMPT and "load_weights" in EXEMPT
    for name, reason in EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 20 and "\n" not in reason, name


def test_every_context_function_of_the_header_is_reached_or_known(driven):
    """The functions no driven method calls are the ones the exempt methods call, and the ones the engine leaves to other modules."""
    reached = {c[0] for c in driven.rec.calls if c[0].startswith("ovn_")}
    elsewhere = {"ovn_abi_version", "ovn_last_error", "ovn_create", "ovn_add_leg_layer", "ovn_finalize",
                 "ovn_set_head_geometry", "ovn_delta_head", "ovn_comm_unique_id", "ovn_comm_init", "ovn_comm_destroy", "ovn_gather_scores"}
    assert set(_lib.SIGNATURES) - reached == elsewhere


def test_the_calls_equal_the_golden_record(driven):
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(driven.rec.calls))
    assert len(got) == len(golden)
    for i, (a, b) in enumerate(zip(got, golden)):
        assert a == b, "entry %d differs from tests/golden/engine_calls.json:\n  now    %s\n  golden %s" % (i, a, b)


def test_refusal_table_covers_every_method_with_tensor_arguments(driven):
    steps = {label: (method, kw) for label, method, kw in driven.steps}
    with_tensors = set()
    for label, method, kw in driven.steps:
        if any(isinstance(v, torch.Tensor) or (isinstance(v, (list, dict)) and any(isinstance(x, torch.Tensor) for x in
                                                                                   (v.values() if isinstance(v, dict) else v)))
               for v in kw.values()):
            with_tensors.add(method)
    refused = {steps[label][0] for label, _, _ in REFUSED}
    assert refused | set(UNCHECKED) == with_tensors, (sorted(with_tensors - refused - set(UNCHECKED)), sorted(refused - with_tensors))
    assert not refused & set(UNCHECKED)


@pytest.mark.parametrize("label,arg,kinds", REFUSED, ids=["%s-%s" % (r[0], r[1]) for r in REFUSED])
def test_bad_tensors_are_refused_before_the_library(driven, label, arg, kinds):
    steps = {l: (method, kw) for l, method, kw in driven.steps}
    method, kw = steps[label]
    rec = driven.rec
    for kind in kinds.split():
        bad = dict(kw)
        bad[arg] = _corrupt(kw[arg], kind)
        before = len(rec.calls)
        try:
            with pytest.raises(_lib.OvnError) as ei:
                driven.invoke(method, bad)
            reached = [c[0] for c in rec.calls[before:] if c[0] not in SIZE_QUERIES]
            assert not reached, "%s(%s: %s) reached %s" % (method, arg, kind, reached)
            assert str(ei.value)
        finally:
            del rec.calls[before:]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["--record"]:
        torch.manual_seed(0)
        with open(GOLDEN, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(c) for c in drive().rec.calls) + "\n]\n")
        print("wrote", GOLDEN)
    else:
        sys.exit("usage: python -m tests.test_engine_calls_host --record")
