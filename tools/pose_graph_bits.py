"""The bits of everything csrc/pose_graph.hip writes, as one SHA-256 per output buffer: what a change that must not move a bit
(a refactor, a compiler update) is compared by.  Run it once per build -- OVN_LIB names the other build -- on the same GPU and
compare the two JSON objects key for key.

Graphs: those of tests._pose_graph_loops_ref.graphs() and a 16-pose chain without loop edges.  Per graph:
  linearize    cost only, then with Jacobians (res, chi, weight, jac, blocks, grad, diag, dinv, chain, record)
  prepare      ovn_pose_graph_loops_prepare: every view of pose_graph_loops_views, and the record
  solve        per preconditioner (jacobi, chain, and loops where there are loop edges) and lambda 0 and 1e-6: 7 iterations at rtol 0,
               then 6 more from first_iteration = 7 (the record after each, delta at the end)
  marginals    both frames, every node and a shuffled subset with one id outside the graph
  retract      the poses moved by the last delta
and, on the two-lap drives of tools/bench_pose_graph.py with 255, 256, 257, 512, 513 and 256^2 + 1 chain edges and two loop edges,
the three preconditioners applied alone to a seeded vector (both precondition entries; the sizes around the scans' block of 256).

ONE JSON object on stdout.

    python tools/pose_graph_bits.py > bits.json"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _pose_graph_loops_ref as LR  # noqa: E402
from tests import _pose_graph_ref as R  # noqa: E402
from tools.bench_pose_graph import drive  # noqa: E402

SCAN_SIZES = (255, 256, 257, 512, 513, 256 * 256 + 1)
LAMBDAS = (0.0, 1e-6)
LIN_KEYS = ("res", "chi", "weight", "jac", "blocks", "grad", "diag", "dinv", "chain")
VIEW_KEYS = ("gamma", "C", "winv", "span", "S", "factor")


def sha(t):
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def upload(eng, g):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    n, e = len(g["init"]), len(g["edges"])
    ptr, lst = R.incidence(n, g["edges"])
    L = e - (n - 1)
    return dict(poses=up(g["init"]), fixed=up(np.asarray(g["fixed"]).astype(np.uint8)), ij=up(np.asarray(g["edges"], np.int32).reshape(e, 2)),
                meas=up(g["Z"].reshape(e, 4, 4)), info=up(g["Omega"].reshape(e, 6, 6)), ptr=up(ptr), lst=up(lst), huber=float(g["huber"]),
                n=n, e=e, L=L, buf=eng.pose_graph_buffers(n, e, chain=True, loops=L))


def linearize(eng, d, jacobians=True):
    return eng.pose_graph_linearize(d["poses"], d["fixed"], d["ij"], d["meas"], d["info"], d["ptr"], d["lst"], d["huber"], d["buf"],
                                    jacobians=jacobians)


def one_graph(eng, name, g, out):
    d = upload(eng, g)
    b, n, L = d["buf"], d["n"], d["L"]
    put = lambda key, t: out.__setitem__("%s/%s" % (name, key), sha(t))
    put("cost_only/record", linearize(eng, d, jacobians=False))
    for k in ("res", "chi", "weight"):
        put("cost_only/" + k, b[k])
    put("linearize/record", linearize(eng, d))
    for k in LIN_KEYS:
        put("linearize/" + k, b[k])
    if L > 0:
        put("prepare/record", eng.pose_graph_loops_prepare(d["poses"], d["ij"], d["info"], b))
        v = eng.pose_graph_loops_views(b, n, L)
        for k in VIEW_KEYS:
            put("prepare/" + k, v[k])
    for kind in ("jacobi", "chain") + (("loops",) if L > 0 else ()):
        for lam in LAMBDAS:
            at = "solve_%s_lam%g" % (kind, lam)
            put(at + "/record_7", eng.pose_graph_solve(d["fixed"], d["ij"], d["ptr"], d["lst"], b, kind, lam, 0.0, 0, 7))
            put(at + "/record_13", eng.pose_graph_solve(d["fixed"], d["ij"], d["ptr"], d["lst"], b, kind, lam, 0.0, 7, 6))
            put(at + "/delta", b["delta"])
    put("retract/poses", eng.pose_graph_retract(d["poses"], d["fixed"], b))
    put("retract/record", b["record"])
    ids = np.random.default_rng(n + L).permutation(n)[:max(n // 3, 2)].astype(np.int32)
    ids[1] = n + 5                                                     # outside the graph: NaNs, counted in slot 15
    queries = {"all": np.arange(n, dtype=np.int32), "subset": ids}
    for frame in ("local", "position"):
        for q, ids in queries.items():
            cov = eng.pose_graph_marginals(d["poses"], b, torch.from_numpy(ids).to(eng.device), L, frame)
            put("marginals_%s_%s/cov" % (frame, q), cov)
            put("marginals_%s_%s/record" % (frame, q), b["record"])


def one_scan_size(eng, n, out):
    """The preconditioners alone on a drive of n chain edges and two loop edges."""
    true, start, edges, Z = drive(n + 1, 2)
    om = np.diag([1.0 / 0.05 ** 2] * 3 + [1.0 / 0.01 ** 2] * 3)
    fixed = np.zeros(n + 1, bool)
    fixed[0] = True
    d = upload(eng, dict(init=start, fixed=fixed, edges=edges, Z=Z, Omega=np.tile(om, (len(edges), 1, 1)), huber=np.inf))
    linearize(eng, d)
    eng.pose_graph_loops_prepare(d["poses"], d["ij"], d["info"], d["buf"])
    y = torch.from_numpy(np.random.default_rng(n).standard_normal((n + 1, 6))).to(eng.device)
    for kind, lam in (("jacobi", 0.5), ("chain", 0.0), ("loops", 0.0)):
        got = eng.pose_graph_precondition(y, d["buf"], kind, lam=lam, out=torch.full_like(y, 7.0), node_ptr=d["ptr"], node_edge=d["lst"])
        out["scan_n%d/precondition_%s" % (n, kind)] = sha(got)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("pose_graph_bits needs the MI355X: there is no CPU path")
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    eng = OvnEngine(64, 900, 1, device=0)
    graphs = dict(LR.graphs())
    chain = R.ring(16, [], seed=5)
    chain["huber"] = np.inf
    graphs["n16_chain"] = chain
    out = {}
    for name, g in graphs.items():
        one_graph(eng, name, g, out)
    for n in SCAN_SIZES:
        one_scan_size(eng, n, out)
    torch.cuda.synchronize()
    eng.close()
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
