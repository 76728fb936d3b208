"""CPU: the C-ABI library builds, loads and exports every symbol include/ovn_hip.h declares; the
product path refuses to run without a GPU (no CPU fallback, nothing under overlapnet_amd imports the oracle)."""
import ctypes
import os
import re

import pytest
import torch

from overlapnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ovn_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_and_exports_header():
    _lib.build()
    assert os.path.isfile(_lib.LIB_PATH)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _header_functions()
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), "libovn_hip.so does not export %s declared in include/ovn_hip.h" % n
    # the Python binding table covers the header one to one
    assert sorted(_lib.SIGNATURES) == names


def _header_text():
    with open(os.path.join(ROOT, "include", "ovn_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8, "unsigned char": ctypes.c_uint8}


def _ctypes_accepted(ctype: str):
    """The ctypes types that may stand for one C parameter or return type of the header."""
    base = " ".join(ctype.replace("const", " ").replace("*", " ").split())
    depth = ctype.count("*")
    if depth == 0:
        return [_SCALARS[base]]
    if base == "ovn_ctx":
        return [ctypes.c_void_p] if depth == 1 else [ctypes.POINTER(ctypes.c_void_p)]
    assert depth == 1, ctype
    if base == "void":
        return [ctypes.c_void_p]
    if base == "char":
        return [ctypes.c_char_p, ctypes.c_void_p]
    return [ctypes.POINTER(_SCALARS[base]), ctypes.c_void_p]


def _header_prototypes():
    """name -> (return type, [parameter types]) as the header spells them, the parameter names dropped."""
    protos = re.findall(r"\b(int|int64_t|const char\*)\s+(ovn_\w+)\s*\(([^;{}]*?)\)\s*;", _header_text(), flags=re.S)
    out = {}
    for ret, name, params in protos:
        types = []
        for p in (" ".join(p.split()) for p in params.split(",")):
            if p == "void":
                continue
            m = re.match(r"^(.*?[\s*])(\w+)$", p)
            assert m, "%s: parameter %r has no name" % (name, p)
            types.append(m.group(1).strip())
        out[name] = (ret, types)
    return out


def test_signatures_have_the_types_of_the_header():
    """A c_int where the header says int64_t, or a c_float for a double, loads and runs and corrupts an argument on the GPU only."""
    protos = _header_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES) and len(protos) >= 84
    wrong = []
    for name, (ret, params) in protos.items():
        res, args = _lib.SIGNATURES[name]
        if res is not (ctypes.c_char_p if "char" in ret else _SCALARS[ret]):
            wrong.append("%s returns %s, SIGNATURES says %s" % (name, ret, res.__name__))
        if len(args) != len(params):
            wrong.append("%s takes %d parameters, SIGNATURES lists %d" % (name, len(params), len(args)))
            continue
        for i, (c, a) in enumerate(zip(params, args)):
            if not any(a is ok for ok in _ctypes_accepted(c)):
                wrong.append("%s parameter %d is %s, SIGNATURES says %s" % (name, i, c, a.__name__))
    assert not wrong, "\n".join(wrong)


def _header_defines():
    """name -> value of every `#define OVN_X <integer>` or `(<integer> << <integer>)`; a define of another form is left out."""
    out = {}
    for name, text in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(OVN_\w+)[ \t]+(\S[^\n]*?)[ \t]*$", _header_text(), flags=re.M):
        m = re.match(r"^\(?\s*(\d+)(?:ll)?\s*(?:<<\s*(\d+)\s*)?\)?$", text)
        if m:
            out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def test_python_constants_equal_the_header_defines():
    from overlapnet_amd import engine, infer, localization, mesh, tsdf, weights
    d = _header_defines()
    assert d["OVN_RENDER_MAX_TRIANGLES"] == 1 << 27 and d["OVN_OK"] == 0            # the evaluator reads both forms
    E = engine.OvnEngine
    mirrored = {
        "OVN_ABI_VERSION": _lib.ABI_VERSION,
        "OVN_SEMANTIC_CLASSES_MAX": engine.SEMANTIC_CLASSES_MAX,
        "OVN_GRAD_PAIR_BLOCK": E.GRAD_PAIR_BLOCK,
        "OVN_LEG_GRAD_SCAN_BLOCK": E.LEG_GRAD_SCAN_BLOCK,
        "OVN_GRAD_REDUCE_MAX_WORLD": E.GRAD_REDUCE_MAX_WORLD,
        "OVN_DELTA_CACHE_ELEMS": E.DELTA_CACHE_ELEMS,
        "OVN_POSE_GRAPH_LOOPS": E.POSE_GRAPH_LOOPS,
        "OVN_POSE_GRAPH_MAX_LOOPS": E.POSE_GRAPH_MAX_LOOPS,
        "OVN_POSE_GRAPH_JACOBI": E.POSE_GRAPH_PRECONDITIONERS["jacobi"],
        "OVN_POSE_GRAPH_CHAIN": E.POSE_GRAPH_PRECONDITIONERS["chain"],
        "OVN_POSE_GRAPH_COV_LOCAL": E.POSE_GRAPH_COV_FRAMES["local"],
        "OVN_POSE_GRAPH_COV_POSITION": E.POSE_GRAPH_COV_FRAMES["position"],
        # the names of slots 0 .. 12, and the three counters behind them: failed pivots [13] and loop edges left out [14] of
        # ovn_pose_graph_loops_prepare, ids out of range [15] of ovn_pose_graph_marginals
        "OVN_POSE_GRAPH_RECORD": len(E.POSE_GRAPH_RECORD) + 3,
        "OVN_TOP_K_MAX": infer.TOP_K_MAX,
        "OVN_RENDER_MAX_TRIANGLES": mesh.MAX_TRIANGLES,
        "OVN_RENDER_LEAF_TRIANGLES": mesh.LEAF_TRIANGLES,
        "OVN_RAYCAST_MAX_SAMPLES": tsdf.MAX_RAY_SAMPLES,
        "OVN_MCL_MAX_PARTICLES": localization.MAX_PARTICLES,
        "OVN_FEAT_W_MIN": weights.FEAT_W_MIN,
        "OVN_FEAT_W_MAX": weights.FEAT_W_MAX,
    }
    assert len(E.POSE_GRAPH_PRECONDITIONERS) == 2 and len(E.POSE_GRAPH_COV_FRAMES) == 2
    wrong = {k: (v, d.get(k)) for k, v in mirrored.items() if d.get(k) != v}
    assert not wrong, "Python constant vs include/ovn_hip.h: %s" % wrong


def test_load_binds_and_versions():
    lib = _lib.load()
    assert lib.ovn_abi_version() == _lib.ABI_VERSION
    assert lib.ovn_last_error() is not None


def test_argument_errors_without_gpu_calls():
    lib = _lib.load()
    # NULL out pointer is rejected before any HIP call
    assert lib.ovn_create(0, 64, 900, 4, None) == 1
    assert b"out is NULL" in lib.ovn_last_error()
    assert lib.ovn_finalize(None, None) == 1
    assert lib.ovn_workspace_bytes(None) == 0
    assert lib.ovn_destroy(None) == 0
    # the optional collective: argument errors before RCCL is even loaded
    assert lib.ovn_comm_unique_id(None) == 1 and b"id_out is NULL" in lib.ovn_last_error()
    assert lib.ovn_comm_init(None, 0, 1, None) == 1
    assert lib.ovn_comm_destroy(None) == 1
    assert lib.ovn_gather_scores(None, None, None, None, 0, None, None, None) != 0 and b"no communicator" in lib.ovn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_product_fails_loudly_without_gpu():
    from overlapnet_amd.engine import OvnEngine
    with pytest.raises(_lib.OvnError):
        OvnEngine(64, 900, 4)
    from overlapnet_amd.infer import Infer
    cfg = {"model": {"leg_output_width": 360, "inputShape": [64, 900], "legsType": "360OutputkLegs",
                     "overlap_head": "DeltaLayerConv1NetworkHead", "orientation_head": "CorrelationHead"},
           "infer_seqs": "x", "data_root_folder": "/tmp", "use_depth": True, "use_normals": True,
           "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False,
           "batch_size": 16, "pretrained_weightsfilename": ""}
    with pytest.raises(_lib.OvnError):
        Infer(cfg)


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "overlapnet_amd")
    for dp, _, fn in os.walk(pkg):
        for f in fn:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                # nor the test / bench infrastructure (synthetic inputs, golden fixtures)
                assert "from tools" not in txt and "import tools" not in txt and "tests/golden" not in txt, f
