"""CPU: the mathematics of the chain-plus-loops inverse as tests/_pose_graph_loops_ref.py states it, what
tests/test_gpu_pose_graph_loops.py builds on, and the refusals of overlapnet_amd.pose_graph and of the library before any GPU work.

Measured here (NumPy fp64): the closed form of S against J H_chain^-1 J' built column by column 1.2e-15 .. 7.4e-15 relative (bound
1e-12); the restated apply against numpy.linalg.solve on the dense Hessian at N = 16 2.3e-15 .. 9.7e-15 relative (bound 1e-9: cond S
is 9e2 .. 3e3 there and cond H about 1e5, times eps, with margin)."""
import json
import os

import numpy as np
import pytest

from tests import _pose_graph_loops_ref as LR
from tests import _pose_graph_ref as R

SMALL = sorted(R.CASES) + ["mixed"]


def _graph(name):
    return LR.mixed() if name == "mixed" else R.case(name)


def _lin(g):
    return R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"])


def test_a_loop_edge_collapses_to_one_block_in_chain_coordinates():
    """A_a N_{i-1} = -B_a N_{j-1}: with A = -B Ad(T_j^-1 T_i) and N_{k-1} = Ad(T_k^-1) both sides are -B Ad(T_j^-1)."""
    rng = np.random.default_rng(0)
    for _ in range(20):
        Ti, Tj = (R.exp_se3(rng.standard_normal(6) * np.array([5.0] * 3 + [1.0] * 3)) for _ in range(2))
        Z = R.mul_se3(R.rel_se3(Ti, Tj), R.exp_se3(0.3 * rng.standard_normal(6)))
        _, A, B = R.edge_terms(Ti, Tj, Z)
        lhs, rhs = A @ R.adjoint(R.inv_se3(Ti)), -B @ R.adjoint(R.inv_se3(Tj))
        assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(rhs).max()


@pytest.mark.parametrize("name", SMALL)
def test_closed_form_of_S_is_J_Hchain_inverse_Jt(name):
    g = _graph(name)
    lin = _lin(g)
    p = LR.prepare(g["init"], lin, g["Omega"])
    L = len(g["edges"]) - (len(g["init"]) - 1)
    want = LR.capacitance_by_columns(g["init"], lin, g["Omega"])
    err = np.abs(p["S"][:6 * L, :6 * L] - want).max() / np.abs(want).max()
    print("POSE_GRAPH_LOOPS %s: S in closed form against J H_chain^-1 J' %.3g" % (name, err))
    assert err <= 1e-12
    assert np.array_equal(p["S"], p["S"].T) and np.array_equal(p["S"][6 * L:], np.eye(len(p["S"]))[6 * L:])
    assert p["pivots"] == 0 and p["left_out"] == 0
    assert np.abs(p["F"] @ p["F"].T - p["S"]).max() <= 1e-13 * np.abs(p["S"]).max()
    assert np.abs(p["F"] - np.linalg.cholesky(p["S"])).max() <= 1e-12 * np.abs(p["F"]).max()


def test_the_mixed_graph_holds_every_kind_of_span():
    spans = [(min(i, j), max(i, j), i > j) for i, j in LR.MIXED_LOOPS]
    assert any(rev for _, _, rev in spans) and any(lo == 0 for lo, _, _ in spans) and any(hi == 15 for _, hi, _ in spans)
    pairs = [(a, b) for k, a in enumerate(spans) for b in spans[k + 1:]]
    assert any(a[0] < b[0] and b[1] < a[1] or b[0] < a[0] and a[1] < b[1] for a, b in pairs), "nested"
    assert any(a[1] <= b[0] or b[1] <= a[0] for a, b in pairs), "disjoint"
    assert any(a[:2] == b[:2] for a, b in pairs), "identical"
    ks = LR._TWO_LAP_KS[:min(LR.TWO_LAP_LOOPS)]
    assert {255, 256, 257} <= set(ks) and all(k < 256 < k + 300 or k < 512 < k + 300 for k in ks)
    assert [6 * L for L in LR.TWO_LAP_LOOPS] == [LR.BLOCK - 6, LR.BLOCK, LR.BLOCK + 6, 2 * LR.BLOCK + 6]


@pytest.mark.parametrize("name", ["n16_loop1", "n16_outlier", "mixed"])
def test_restated_apply_is_the_inverse_of_the_dense_hessian(name):
    g = _graph(name)
    lin = _lin(g)
    H, free = R.dense_system(lin, 0.0)
    y = np.zeros((16, 6))
    y[1:] = np.random.default_rng(3).standard_normal((15, 6))
    want = np.linalg.solve(H, y[1:].ravel()).reshape(-1, 6)
    for reverse in (False, True):
        z = LR.apply(LR.prepare(g["init"], lin, g["Omega"], reverse), y, reverse)
        err = np.abs(z[1:] - want).max() / np.abs(want).max()
        print("POSE_GRAPH_LOOPS %s: the restated apply against the dense solve %.3g (reversed sums: %s)" % (name, err, reverse))
        assert np.all(z[0] == 0.0) and err <= 1e-9


def test_scan_orders_agree_across_blocks():
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 513):
        v = rng.standard_normal((n, 6))
        a, b, c = LR.scan(v), LR.scan(v, reverse=True), np.cumsum(v, axis=0)
        assert np.abs(a - c).max() <= 1e-12 * max(1.0, np.abs(c).max()) and np.abs(b - c).max() <= 1e-12 * max(1.0, np.abs(c).max())


def test_blocked_cholesky_and_its_sweeps():
    rng = np.random.default_rng(6)
    for sp in (48, 96, 144):
        A = rng.standard_normal((sp, sp))
        S = A @ A.T + sp * np.eye(sp)
        v = rng.standard_normal(sp)
        for reverse in (False, True):
            F, fails = LR.cholesky_blocked(S, reverse=reverse)
            assert fails == 0 and np.abs(F - np.linalg.cholesky(S)).max() <= 1e-12 * np.abs(F).max()
            assert np.abs(LR.solve_factor(F, v, reverse=reverse) - np.linalg.solve(S, v)).max() <= 1e-12
    S[5, 5] = -1.0
    with np.errstate(all="ignore"):
        F, fails = LR.cholesky_blocked(S)                            # counted, 1 in the pivot's place; what follows it is not promised
    assert fails >= 1 and np.isfinite(F[:6]).all()


@pytest.mark.parametrize("name", SMALL)
def test_restated_pcg_converges_in_one_iteration_undamped_and_matches_the_golden_counts(name):
    g = _graph(name)
    lin = _lin(g)
    got = LR.golden_entry(g, lin)
    assert got["lam0"]["iterations"] == 1
    assert got["lam0"]["dense_distance"] <= 1e-12 and got["lam1e-6"]["dense_distance"] <= 1e-8
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_loops.json")))
    assert sorted(gold) == sorted(LR.graphs()) if name == SMALL[0] else True
    for key in LR.LAMBDAS:
        assert gold[name][key]["iterations"] == got[key]["iterations"]
        assert 0.5 * gold[name][key]["dense_distance"] <= got[key]["dense_distance"] <= 2.0 * gold[name][key]["dense_distance"] \
            or abs(gold[name][key]["dense_distance"] - got[key]["dense_distance"]) <= 1e-14
    # damped, it is a preconditioner: never worse than the chain
    pre_chain = R.make_precond("chain", g["init"], lin, g["Omega"], 1e-6)
    _, it_chain, _ = R.pcg(lin, 1e-6, pre_chain, 1e-8, 500)
    assert got["lam1e-6"]["iterations"] <= it_chain


def test_a_loop_edge_of_weight_zero_is_left_out():
    g = R.case("n16_outlier")
    Z = g["Z"].copy()
    Z[-1, 1, 2] = np.nan
    lin = R.linearize(g["init"], g["fixed"], g["edges"], Z, g["Omega"], g["huber"])
    p = LR.prepare(g["init"], lin, g["Omega"])
    assert p["left_out"] == 1 and p["pivots"] == 0 and np.all(p["C"][-1] == 0) and np.all(p["span"][-1] == 0)
    assert np.array_equal(p["S"][12:18, :18], np.eye(18)[12:18])
    keep = np.arange(len(g["edges"]) - 1)
    lin2 = R.linearize(g["init"], g["fixed"], g["edges"][keep], Z[keep], g["Omega"][keep], g["huber"])
    y = np.zeros((16, 6))
    y[1:] = np.random.default_rng(7).standard_normal((15, 6))
    H, _ = R.dense_system(lin2, 0.0)
    want = np.linalg.solve(H, y[1:].ravel()).reshape(-1, 6)
    assert np.abs(LR.apply(p, y)[1:] - want).max() <= 1e-9 * np.abs(want).max()


def test_python_refusals_and_the_selectors():
    from overlapnet_amd import pose_graph as PG
    om = PG.information_from_sigmas(0.05, 0.01)
    poses = np.stack([np.eye(4)] * 64)
    c = PG.PoseGraph(None, poses)
    c.add_odometry(poses, om)
    assert c.loops == 0 and c.fallbacks == 0
    with pytest.raises(ValueError, match="1 .. %d loop edges" % PG.MAX_LOOPS):
        c.choose_preconditioner("loops")                             # L = 0
    assert c.choose_preconditioner("auto+loops") == c.choose_preconditioner("auto") == "chain"
    c.add_edge(63, 0, np.eye(4), om)
    assert c.loops == 1 and c.choose_preconditioner("loops") == "loops" and c.choose_preconditioner("auto") == "chain"
    assert c.choose_preconditioner("auto+loops") == ("loops" if PG.LOOPS_MIN <= 1 else "chain")
    d = PG.PoseGraph(None, poses, fixed=(0, 2))                      # the chain precondition fails: two fixed nodes
    d.add_odometry(poses, om)
    d.add_edge(63, 0, np.eye(4), om)
    with pytest.raises(ValueError, match="chain-plus-loops inverse needs"):
        d.choose_preconditioner("loops")
    assert d.choose_preconditioner("auto+loops") == d.choose_preconditioner("auto") == "jacobi"
    r = PG.PoseGraph(None, poses)                                    # loop edges first: not a chain
    r.add_edge(4, 0, np.eye(4), om)
    r.add_odometry(poses, om)
    with pytest.raises(ValueError, match="chain-plus-loops inverse needs"):
        r.choose_preconditioner("loops")
    with pytest.raises(ValueError, match="no preconditioner"):
        c.choose_preconditioner("loops+auto")
    big = PG.PoseGraph(None, poses)
    big.add_odometry(poses, om)
    big._ij += [(40, 3)] * (PG.MAX_LOOPS + 1)                        # past add_edge, for speed
    assert big.loops == PG.MAX_LOOPS + 1
    with pytest.raises(ValueError, match="the graph has %d" % (PG.MAX_LOOPS + 1)):
        big.choose_preconditioner("loops")
    assert big.choose_preconditioner("auto+loops") == big.choose_preconditioner("auto")
    big._ij.pop()
    assert big.choose_preconditioner("loops") == "loops" and big.choose_preconditioner("auto+loops") == "loops"


def test_auto_plus_loops_rule_and_auto_unchanged():
    from overlapnet_amd import pose_graph as PG
    om = PG.information_from_sigmas(0.05, 0.01)
    poses = np.stack([np.eye(4)] * 64)
    g = PG.PoseGraph(None, poses)
    g.add_odometry(poses, om)
    seen = []
    for k in range(31):
        g.add_edge(62 - k, k + 1, np.eye(4), om) if k else g.add_edge(63, 0, np.eye(4), om)
        want_auto = "chain" if 6 * g.loops + 1 < PG.JACOBI_ITERATIONS_PER_NODE * 64 else "jacobi"
        assert g.choose_preconditioner("auto") == want_auto          # today's rule, to the letter
        want = "loops" if PG.LOOPS_MIN <= g.loops <= PG.MAX_LOOPS else want_auto
        assert g.choose_preconditioner("auto+loops") == want
        seen.append(want_auto)
    assert seen[0] == "chain" and seen[-1] == "jacobi"
    assert 1 <= PG.LOOPS_MIN <= PG.MAX_LOOPS == LR.MAX_LOOPS


def test_library_limits_and_argument_errors_need_no_gpu():
    import ctypes as C
    import re
    from overlapnet_amd import _lib
    from overlapnet_amd import pose_graph as PG
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ovn_hip.h")).read()
    cap = int(re.search(r"#define OVN_POSE_GRAPH_MAX_LOOPS (\d+)\n#endif", header).group(1))
    assert cap == PG.MAX_LOOPS == LR.MAX_LOOPS and re.search(r"#define OVN_POSE_GRAPH_LOOPS 2\b", header)
    f = lib.ovn_pose_graph_loops_bytes
    assert f(2, 1) > 0 and f(1 << 20, cap) > 0
    assert f(1, 1) == 0 and f((1 << 20) + 1, 1) == 0 and f(16, 0) == 0 and f(16, -1) == 0 and f(16, cap + 1) == 0
    assert f(600, 9) > f(600, 8) >= f(600, 7) > 0                    # 6 L = 42 and 48 share one block of 48, 54 takes two
    sp = lambda L: (6 * L + LR.BLOCK - 1) // LR.BLOCK * LR.BLOCK
    assert f(16, cap) >= 2 * 8 * sp(cap) ** 2
    lay = (C.c_int64 * 8)()
    assert lib.ovn_pose_graph_loops_layout(600, 9, lay) == 0 and lay[0] == LR.BLOCK and lay[1] == 96 and lay[2] == 0
    assert list(lay[2:8]) == sorted(lay[2:8]) and 8 * (lay[7] + 96 * 96) <= f(600, 9)
    assert lib.ovn_pose_graph_loops_layout(600, cap + 1, lay) == 1 and lib.ovn_pose_graph_loops_layout(600, 9, None) == 1
    assert lib.ovn_pose_graph_loops_prepare(None, None, None, 4, None, None, None, None, 4, 1, None, 7, None, None) == 1
    assert b"ctx is NULL" in lib.ovn_last_error()
    assert lib.ovn_pose_graph_solve_loops(None, None, None, 4, None, 4, *([None] * 8), 1, 0.0, 1e-8, 0, 1, None, None, None) == 1
    assert lib.ovn_pose_graph_precondition_loops(None, None, 4, 4, 1, *([None] * 7)) == 1


def test_slam_tool_offers_the_new_selectors():
    from tools import slam
    base = ["--config", "c.json", "--scans", "s", "--out", "o.txt", "--overlap-thres", "0.3", "--min-fitness", "none", "--max-rms", "0.1",
            "--odom-sigma", "0.05", "0.01", "--loop-sigma", "0.1", "0.02", "--huber", "None"]
    assert slam.parse(base).preconditioner == "auto"
    for kind in ("loops", "auto+loops"):
        assert slam.parse(base + ["--preconditioner", kind]).preconditioner == kind
