"""GPU (MI355X): the chain-plus-loops inverse (ovn_pose_graph_loops_*, csrc/pose_graph.hip) against its NumPy
statement (tests/_pose_graph_loops_ref.py).

Graphs (LR.graphs): the three cases of tests/_pose_graph_ref.py (L = 1, 3 with a Huber-weighted outlier, 2); `mixed`, 16 poses with
loop edges that have i > j, touch node 0, end at node N - 1, and whose spans are nested, disjoint and identical; and a two-lap ring of
600 poses with L = 7, 8, 9, 17 loop edges (k + 300, k) -- 6 L = 42, 48, 54, 102 is one 6-block under, on and over the factorization's
block size 48, and 2 * 48 + 6 -- whose first k are 255, 256, 257 and whose spans all cross the scans' block boundary at 256 or 512.

Tolerances.  The kernels take the restatement's sums in the restatement's order, so what separates the two is libm in the
linearization and nothing else that is known.  The allowance for Gamma, C, S, the factor, the apply and delta after two iterations is
measured on the restatement itself: ten times its distance from its own form with every sum reversed, relative to the quantity's
largest magnitude (printed per graph; where that distance is 0 the GPU has to agree to the bit).  Two iterations are taken at lambda
= 1e-6: at lambda = 0 the first iteration already converges (the inverse is exact) and a second one would work on rounding noise.
Convergence: the restatement's iteration counts to rtol 1e-8 and its distance from numpy.linalg.solve at lambda = 0 and 1e-6 are
tests/golden/pose_graph_loops.json (python -m tests._pose_graph_loops_ref); the GPU may take two iterations more and lie ten times as
far from the dense solve.  optimize: the bound of tests/test_gpu_pose_graph.py, ten times OPT_FIGURE = 1.4e-9 against the
reference run with a dense solve."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _pose_graph_loops_ref as LR
from tests import _pose_graph_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

OPT_FIGURE = 1.4e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_loops.json")
NAMES = sorted(R.CASES) + ["mixed"] + ["two_lap_L%d" % L for L in LR.TWO_LAP_LOOPS]
SMALL = sorted(R.CASES) + ["mixed"]


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    e = OvnEngine(64, 900, 1, device=0)
    yield e
    torch.cuda.synchronize()
    e.close()


def _lin(g, reverse=False):
    return R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], reverse=reverse)


@pytest.fixture(scope="module")
def ref():
    """Per graph: the graph, its reference linearization and the restated prepare, forward and with reversed sums."""
    gs = LR.graphs()
    big = LR.two_lap()
    big_lin = _lin(big)
    out = {}
    for name, g in gs.items():
        lin = LR.restrict(big_lin, len(g["edges"])) if name.startswith("two_lap") else _lin(g)
        out[name] = dict(g=g, lin=lin, fwd=LR.prepare(g["init"], lin, g["Omega"]), rev=LR.prepare(g["init"], lin, g["Omega"], True),
                         loops=len(g["edges"]) - (len(g["init"]) - 1))
    out["golden"] = json.load(open(GOLDEN))
    return out


def _up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _graph(eng, g, loops=True):
    n, e = len(g["init"]), len(g["edges"])
    ptr, lst = R.incidence(n, g["edges"])
    return dict(poses=_up(eng, g["init"]), fixed=_up(eng, g["fixed"].astype(np.uint8)), ij=_up(eng, g["edges"].astype(np.int32).reshape(e, 2)),
                meas=_up(eng, g["Z"].reshape(e, 4, 4)), info=_up(eng, g["Omega"].reshape(e, 6, 6)), ptr=_up(eng, ptr), lst=_up(eng, lst),
                huber=g["huber"], n=n, e=e, loops=e - (n - 1), buf=eng.pose_graph_buffers(n, e, loops=e - (n - 1)) if loops else None)


def _prepare(eng, d):
    eng.pose_graph_linearize(d["poses"], d["fixed"], d["ij"], d["meas"], d["info"], d["ptr"], d["lst"], d["huber"], d["buf"])
    return eng.pose_graph_loops_prepare(d["poses"], d["ij"], d["info"], d["buf"]).cpu().numpy()


def _solve(eng, d, lam=0.0, rtol=1e-8, first=0, iters=8, kind="loops"):
    return eng.pose_graph_solve(d["fixed"], d["ij"], d["ptr"], d["lst"], d["buf"], kind, lam, rtol, first, iters).cpu().numpy()


def _rel(a, b):
    b = np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (scale if scale > 0 else 1.0))


@pytest.mark.parametrize("name", NAMES)
def test_prepare(eng, ref, name):
    c = ref[name]
    g, fwd, rev, L = c["g"], c["fwd"], c["rev"], c["loops"]
    d = _graph(eng, g)
    rec = _prepare(eng, d)
    v = {k: (t.cpu().numpy() if torch.is_tensor(t) else t) for k, t in eng.pose_graph_loops_views(d["buf"], d["n"], L).items()}
    assert v["block"] == LR.BLOCK and v["sp"] == len(fwd["S"]) and v["sp"] % LR.BLOCK == 0 and 0 <= v["sp"] - 6 * L < LR.BLOCK
    assert rec[13] == 0 and rec[14] == 0 and fwd["pivots"] == 0 and fwd["left_out"] == 0
    assert np.array_equal(v["span"], fwd["span"])
    got = dict(gamma=v["gamma"], C=v["C"], S=v["S"], F=np.tril(v["factor"]))
    for k, a in got.items():
        fig, err = _rel(rev[k], fwd[k]), _rel(a, fwd[k])
        print("POSE_GRAPH_LOOPS %s: %-5s the restatement against its reversed sums %.3g, the GPU against the restatement %.3g%s"
              % (name, k, fig, err, " (the same bits)" if np.array_equal(a, fwd[k]) else ""))
    for k, a in got.items():
        assert _rel(a, fwd[k]) <= 10 * _rel(rev[k], fwd[k]), k
    G = d["buf"]["chain"][:, 0].cpu().numpy()                          # no libm between the G the GPU holds and its Gamma
    assert np.array_equal(v["gamma"], LR.gamma(G)), "Gamma is the scan of G in the scans' order of additions, to the bit"
    assert np.array_equal(v["S"], v["S"].T), "S is symmetric by construction"
    assert np.all(np.triu(v["factor"], 1) == 0)
    pad = slice(6 * L, v["sp"])
    eye = np.eye(v["sp"])
    assert np.array_equal(v["S"][pad], eye[pad]) and np.array_equal(v["factor"][pad], eye[pad])
    assert _rel(got["F"] @ got["F"].T, v["S"]) <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_precondition_alone(eng, ref, name):
    c = ref[name]
    g, n = c["g"], len(c["g"]["init"])
    y = np.random.default_rng(n + c["loops"]).standard_normal((n, 6))
    want, back = LR.apply(c["fwd"], y), LR.apply(c["rev"], y, True)
    d = _graph(eng, g)
    _prepare(eng, d)
    out = torch.full((n, 6), 7.0, dtype=torch.float64, device=eng.device)
    got = eng.pose_graph_precondition(_up(eng, y), d["buf"], "loops", out=out, node_ptr=d["ptr"], node_edge=d["lst"]).cpu().numpy()
    fig, err = _rel(back, want), _rel(got, want)
    print("POSE_GRAPH_LOOPS %s: H^-1 y, the restatement against its reversed sums %.3g, the GPU against the restatement %.3g%s"
          % (name, fig, err, " (the same bits)" if np.array_equal(got, want) else ""))
    assert np.all(got[0] == 0.0)
    assert err <= 10 * fig
    if name in SMALL:                                                # and it IS the inverse: against the dense Hessian
        H, free = R.dense_system(c["lin"], 0.0)
        dense = np.linalg.solve(H, y[1:].ravel()).reshape(-1, 6)
        assert _rel(got[1:], dense) <= 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_delta_after_two_iterations(eng, ref, name):
    c, lam = ref[name], 1e-6
    g, lin = c["g"], c["lin"]
    want, it, _ = R.pcg(lin, lam, lambda r: LR.apply(c["fwd"], r), 0.0, 2)
    back, itb, _ = R.pcg(lin, lam, lambda r: LR.apply(c["rev"], r, True), 0.0, 2, reverse=True)
    assert it == 2 and itb == 2
    d = _graph(eng, g)
    _prepare(eng, d)
    rec = _solve(eng, d, lam, rtol=0.0, iters=2)
    got = d["buf"]["delta"].cpu().numpy()
    fig, err = _rel(back, want), _rel(got, want)
    print("POSE_GRAPH_LOOPS %s: delta after 2 iterations at lambda 1e-6, the restatement against its reversed sums %.3g, the GPU "
          "against the restatement %.3g, record %s" % (name, fig, err, rec[4:8]))
    assert rec[4] == 2 and rec[7] == 0
    assert np.all(got[g["fixed"]] == 0)
    assert err <= 10 * fig


@pytest.mark.parametrize("key", sorted(LR.LAMBDAS))
@pytest.mark.parametrize("name", NAMES)
def test_convergence(eng, ref, name, key):
    c, lam, gold = ref[name], LR.LAMBDAS[key], ref["golden"][name][key]
    d = _graph(eng, c["g"])
    _prepare(eng, d)
    rec = _solve(eng, d, lam, iters=gold["iterations"] + 2)
    got = d["buf"]["delta"].cpu().numpy()
    dense = R.dense_solve(c["lin"], lam)
    err = float(np.abs(got - dense).max())
    print("POSE_GRAPH_LOOPS %s %s: converged after %d iterations (the restatement: %d) at %.3g, |delta - dense|_inf %.3g (the "
          "restatement: %.3g)" % (name, key, rec[4], gold["iterations"], rec[5], err, gold["dense_distance"]))
    assert rec[6] == 1 and rec[7] == 0 and rec[5] <= 1e-8
    assert rec[4] <= gold["iterations"] + 2
    if lam == 0.0 and name in SMALL:
        assert rec[4] == 1                                           # the inverse is exact
    assert err <= 10 * gold["dense_distance"]


def _pose_graph(eng, g):
    from overlapnet_amd.pose_graph import PoseGraph
    pg = PoseGraph(eng, g["init"], fixed=np.flatnonzero(g["fixed"]))
    for (i, j), Z, om in zip(g["edges"], g["Z"], g["Omega"]):
        pg.add_edge(i, j, Z, om)
    return pg


@pytest.mark.parametrize("kind", ["loops", "auto+loops"])
@pytest.mark.parametrize("name", SMALL)
def test_optimize(eng, ref, name, kind):
    g = ref[name]["g"]
    want = R.optimize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], max_iterations=30, solver="dense")
    assert want["converged"]
    pg = _pose_graph(eng, g)
    assert pg.choose_preconditioner(kind) == "loops"
    res = pg.optimize(huber=None if np.isinf(g["huber"]) else g["huber"], preconditioner=kind)
    err = float(np.abs(res.poses - want["poses"]).max())
    print("POSE_GRAPH_LOOPS %s %s: %d outer / %d PCG iterations, cost %.10g -> %.10g (reference %.10g in %d), poses within %.3g (bound "
          "%.3g), fallbacks %d" % (name, kind, res.outer_iterations, res.cg_iterations, res.cost_initial, res.cost_final,
                                   want["cost_final"], want["outer_iterations"], err, 10 * OPT_FIGURE, pg.fallbacks))
    assert res.converged and res.outer_iterations <= 30 and pg.fallbacks == 0
    assert err <= 10 * OPT_FIGURE
    assert abs(res.cost_final - want["cost_final"]) <= 1e-9 * want["cost_final"]
    assert np.array_equal(res.poses[0], g["init"][0])
    if name == "n16_outlier":
        assert res.weights[-1] < 0.02 and np.all(res.weights[:-1] == 1.0)
    else:
        assert np.all(res.weights == 1.0)


def test_a_nan_loop_measurement_is_left_out_and_counted(eng, ref):
    g = dict(ref["n16_outlier"]["g"])
    g["Z"] = g["Z"].copy()
    g["Z"][-1, 1, 2] = np.nan                                        # the outlier edge (4, 11), the last loop edge
    d = _graph(eng, g)
    rec = _prepare(eng, d)
    assert rec[1] == 1 and rec[13] == 0 and rec[14] == 1
    v = eng.pose_graph_loops_views(d["buf"], d["n"], d["loops"])
    S = v["S"].cpu().numpy()
    assert np.all(v["C"][-1].cpu().numpy() == 0) and np.all(v["span"][-1].cpu().numpy() == 0)
    assert np.array_equal(S[12:18, :18], np.eye(18)[12:18]) and np.isfinite(S).all() and np.isfinite(v["factor"].cpu().numpy()).all()
    rec = _solve(eng, d)
    got = d["buf"]["delta"].cpu().numpy()
    assert rec[6] == 1 and rec[7] == 0 and rec[4] <= 1 + 2 and np.isfinite(got).all()
    keep = np.arange(len(g["edges"]) - 1)                            # the graph without that edge
    lin = R.linearize(g["init"], g["fixed"], g["edges"][keep], g["Z"][keep], g["Omega"][keep], g["huber"])
    assert np.abs(got - R.dense_solve(lin, 0.0)).max() <= 1e-9 * np.abs(got).max()


def test_zero_information_on_a_loop_edge_breaks_down_and_optimize_falls_back(eng, ref):
    g = dict(ref["n16_loop1"]["g"])
    g["Omega"] = g["Omega"].copy()
    g["Omega"][-1] = 0.0
    d = _graph(eng, g)
    rec = _prepare(eng, d)
    assert rec[2] == 0 and rec[13] == 1 and rec[14] == 0
    d["buf"]["delta"].fill_(7.0)
    rec = _solve(eng, d, iters=4)
    assert rec[7] == 1 and rec[6] == 0 and rec[4] == 0
    assert np.all(d["buf"]["delta"].cpu().numpy() == 7.0)
    from overlapnet_amd.pose_graph import PoseGraph
    runs = {}
    for kind in ("loops", "chain"):
        pg = PoseGraph(eng, g["init"])
        pg._ij, pg._z, pg._info = [tuple(e) for e in g["edges"]], list(g["Z"]), list(g["Omega"])     # past add_edge's refusal
        runs[kind] = (pg, pg.optimize(preconditioner=kind))
    pg, res = runs["loops"]
    assert res.converged and pg.fallbacks == res.outer_iterations > 0 and runs["chain"][0].fallbacks == 0
    assert np.array_equal(res.poses, runs["chain"][1].poses)


def test_same_arguments_same_bits(eng, ref):
    g = ref["two_lap_L9"]["g"]
    bits = lambda x: np.ascontiguousarray(x).view(np.int64)
    runs = []
    for _ in range(2):
        d = _graph(eng, g)
        rec = [_prepare(eng, d).copy()]
        loops = d["buf"]["loops"].cpu().numpy().copy()
        rec.append(_solve(eng, d, 1e-6, rtol=0.0, iters=7).copy())
        rec.append(_solve(eng, d, 1e-6, rtol=0.0, first=7, iters=6).copy())
        delta = d["buf"]["delta"].cpu().numpy().copy()
        pre = eng.pose_graph_precondition(d["buf"]["grad"], d["buf"], "loops", node_ptr=d["ptr"], node_edge=d["lst"]).cpu().numpy()
        lay = eng.pose_graph_loops_views(d["buf"], d["n"], d["loops"])
        runs.append((rec, [lay[k].cpu().numpy().copy() for k in ("gamma", "C", "winv", "span", "S", "factor")], delta, pre))
    a, b = runs
    for x, y in zip(a[0] + a[1] + [a[2], a[3]], b[0] + b[1] + [b[2], b[3]]):
        assert np.array_equal(bits(x), bits(y))
    d = _graph(eng, g)                                               # 7 + 6 iterations in two chunks are 13 in one
    _prepare(eng, d)
    one = _solve(eng, d, 1e-6, rtol=0.0, iters=13)
    assert one[4] == a[0][2][4] and np.array_equal(bits(one), bits(a[0][2]))
    assert np.array_equal(bits(d["buf"]["delta"].cpu().numpy()), bits(a[2]))


def test_argument_errors(eng, ref):
    g = ref["n16_outlier"]["g"]
    d = _graph(eng, g)
    _prepare(eng, d)
    _solve(eng, d, iters=1)
    lib, h, s = eng.lib, eng._h, eng._stream()
    p = lambda t: None if t is None else t.data_ptr()
    b = d["buf"]
    n, e, L = d["n"], d["e"], d["loops"]
    out = torch.zeros((n, 6), dtype=torch.float64, device=eng.device)
    before = {k: v.clone() for k, v in b.items()}

    def prep(**kw):
        a = dict(poses=p(d["poses"]), n=n, ij=p(d["ij"]), info=p(d["info"]), weight=p(b["weight"]), jac=p(b["jac"]), e=e, L=L,
                 chain=p(b["chain"]), stages=7, loops=p(b["loops"]), rec=p(b["record"]))
        a.update(kw)
        return lib.ovn_pose_graph_loops_prepare(h, s, a["poses"], a["n"], a["ij"], a["info"], a["weight"], a["jac"], a["e"], a["L"],
                                                a["chain"], a["stages"], a["loops"], a["rec"])

    def solve(**kw):
        a = dict(fixed=p(d["fixed"]), n=n, ij=p(d["ij"]), e=e, ptr=p(d["ptr"]), lst=p(d["lst"]), blocks=p(b["blocks"]), grad=p(b["grad"]),
                 diag=p(b["diag"]), dinv=p(b["dinv"]), chain=p(b["chain"]), loops=p(b["loops"]), L=L, lam=0.0, rtol=1e-8, first=0, iters=4,
                 delta=p(b["delta"]), ws=p(b["ws"]), rec=p(b["record"]))
        a.update(kw)
        return lib.ovn_pose_graph_solve_loops(h, s, a["fixed"], a["n"], a["ij"], a["e"], a["ptr"], a["lst"], a["blocks"], a["grad"],
                                              a["diag"], a["dinv"], a["chain"], a["loops"], a["L"], a["lam"], a["rtol"], a["first"],
                                              a["iters"], a["delta"], a["ws"], a["rec"])

    def pre(**kw):
        a = dict(n=n, e=e, L=L, ptr=p(d["ptr"]), lst=p(d["lst"]), chain=p(b["chain"]), loops=p(b["loops"]), i=p(b["grad"]), o=p(out),
                 ws=p(b["ws"]))
        a.update(kw)
        return lib.ovn_pose_graph_precondition_loops(h, s, a["n"], a["e"], a["L"], a["ptr"], a["lst"], a["chain"], a["loops"], a["i"],
                                                     a["o"], a["ws"])

    shape = [dict(n=1, e=L), dict(n=(1 << 20) + 1), dict(L=0, e=n - 1), dict(L=-1), dict(L=LR.MAX_LOOPS + 1, e=n + LR.MAX_LOOPS),
             dict(e=e + 1), dict(e=e - 1), dict(L=L + 1), dict(L=L - 1)]
    for kw in shape + [dict(poses=None), dict(ij=None), dict(info=None), dict(weight=None), dict(jac=None), dict(chain=None),
                       dict(loops=None), dict(rec=None), dict(stages=0), dict(stages=8)]:
        assert prep(**kw) == 1, kw
        assert lib.ovn_last_error()
    for kw in shape + [dict(lam=-1e-3), dict(lam=float("inf")), dict(lam=float("nan")), dict(rtol=-1.0), dict(rtol=float("nan")),
                       dict(first=-1), dict(iters=-1), dict(iters=4097), dict(rec=None), dict(ws=None), dict(delta=None), dict(fixed=None),
                       dict(ij=None), dict(ptr=None), dict(lst=None), dict(blocks=None), dict(grad=None), dict(diag=None), dict(dinv=None),
                       dict(chain=None), dict(loops=None)]:
        assert solve(**kw) == 1, kw
    for kw in shape + [dict(ptr=None), dict(lst=None), dict(chain=None), dict(loops=None), dict(i=None), dict(o=None), dict(ws=None)]:
        assert pre(**kw) == 1, kw
    assert lib.ovn_pose_graph_solve(h, s, p(d["fixed"]), n, p(d["ij"]), e, p(d["ptr"]), p(d["lst"]), p(b["blocks"]), p(b["grad"]),
                                    p(b["diag"]), p(b["dinv"]), p(b["chain"]), 2, 0.0, 1e-8, 0, 4, p(b["delta"]), p(b["ws"]),
                                    p(b["record"])) == 1               # OVN_POSE_GRAPH_LOOPS is not served by the older entry
    torch.cuda.synchronize()
    for k, v in b.items():
        assert torch.equal(v.view(torch.int64), before[k].view(torch.int64)), "a refused call wrote %s" % k
    assert np.all(out.cpu().numpy() == 0)
    assert prep() == 0 and solve() == 0 and pre() == 0
    torch.cuda.synchronize()
    from overlapnet_amd._lib import OvnError
    with pytest.raises(OvnError, match="loops="):
        eng.pose_graph_solve(d["fixed"], d["ij"], d["ptr"], d["lst"], eng.pose_graph_buffers(n, e, chain=True), "loops")
    with pytest.raises(OvnError, match="loop edges"):
        eng.pose_graph_buffers(n, n - 1, loops=1)
