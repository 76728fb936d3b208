"""CPU: the NumPy statement of the pose-graph optimizer (tests/_pose_graph_ref.py) holds what tests/test_gpu_pose_graph.py builds on,
and overlapnet_amd.pose_graph refuses a malformed graph before any GPU work."""
import numpy as np
import pytest

from tests import _pose_graph_ref as R

ANGLES = (0.0, 1e-9, 1e-4, 0.05, 0.0999, 0.1001, 0.5, 1.0, 2.0)     # both sides of the series switch-over at theta = 0.1


def _twist(rng, theta):
    w = rng.standard_normal(3)
    return np.concatenate([rng.standard_normal(3), w / np.linalg.norm(w) * theta])


def test_exp_log_round_trip():
    rng = np.random.default_rng(0)
    for th in ANGLES + (3.0,):
        xi = _twist(rng, th)
        T = R.exp_se3(xi)
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() < 4e-16 * 4
        assert np.abs(R.log_se3(T) - xi).max() < 1e-14 * max(1.0, np.abs(xi).max())
        assert np.abs(R.mul_se3(T, R.exp_se3(-xi)) - np.eye(4)).max() < 1e-14 * max(1.0, np.abs(xi).max())


def test_coefficient_series_meet_the_closed_forms_at_the_switch():
    x = R.SERIES_X
    below, above = np.array(R.coeffs(np.nextafter(x, 0.0))), np.array(R.coeffs(x))
    # the closed forms cancel: c3's numerator 2 t - 3 sin t + t cos t is t^5 / 60 formed from terms of size 2 t, so one rounding of a
    # term is 120 eps / t^4 of the result -- the worst of the six; the series' own truncation (x^5 terms) is below 1e-17
    assert np.abs(below / above - 1.0).max() < 120 * np.finfo(np.float64).eps / x ** 2


def _numeric(Ti, Tj, Z, h=1e-6):
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        p, m = R.exp_se3(d), R.exp_se3(-d)
        A[:, k] = (R.residual(R.mul_se3(Ti, p), Tj, Z) - R.residual(R.mul_se3(Ti, m), Tj, Z)) / (2 * h)
        B[:, k] = (R.residual(Ti, R.mul_se3(Tj, p), Z) - R.residual(Ti, R.mul_se3(Tj, m), Z)) / (2 * h)
    return A, B


@pytest.mark.parametrize("theta", ANGLES)
def test_jacobians_against_central_differences(theta):
    rng = np.random.default_rng(int(theta * 1e6) + 1)
    for _ in range(4):
        Ti, Tj = R.exp_se3(_twist(rng, 2.0 * rng.random())), R.exp_se3(_twist(rng, 2.0 * rng.random()))
        Z = R.mul_se3(R.rel_se3(Ti, Tj), R.exp_se3(-_twist(rng, theta)))          # the residual's rotation is theta
        r, A, B = R.edge_terms(Ti, Tj, Z)
        assert abs(np.linalg.norm(r[3:]) - theta) < 1e-9
        An, Bn = _numeric(Ti, Tj, Z)
        assert np.abs(A - An).max() <= 1e-6 * np.abs(A).max()
        assert np.abs(B - Bn).max() <= 1e-6 * np.abs(B).max()


def test_chain_preconditioner_is_the_inverse_of_the_chain_hessian():
    g = R.ring(16, [], seed=3)
    lin = R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"])
    H, free = R.dense_system(lin, 0.0)
    assert list(free) == list(range(1, 16))
    G, N = R.chain_terms(g["init"], lin, g["Omega"])
    y = np.zeros((16, 6))
    y[1:] = np.random.default_rng(4).standard_normal((15, 6))
    want = np.linalg.solve(H, y[1:].ravel()).reshape(-1, 6)
    for apply in (R.chain_apply, R.chain_apply_scan):
        z = apply(G, N, y)
        assert np.all(z[0] == 0.0)
        assert np.abs(z[1:] - want).max() <= 1e-10 * np.abs(want).max()          # cond(H) is about 1e5 here


def test_chain_scan_order_straddles_blocks():
    rng = np.random.default_rng(5)
    for n in (255, 256, 257, 513):
        G, N = rng.standard_normal((n, 6, 6)), rng.standard_normal((n, 6, 6))
        y = rng.standard_normal((n + 1, 6))
        a, b = R.chain_apply(G, N, y), R.chain_apply_scan(G, N, y)
        assert np.abs(a - b).max() <= 1e-11 * np.abs(a).max()


def test_pcg_iteration_counts_and_solution():
    g = R.case("n16_loop1")
    lin = R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"])
    xd = R.dense_solve(lin, 0.0)
    x, it, rel = R.pcg(lin, 0.0, R.make_precond("chain", g["init"], lin, g["Omega"], 0.0), 1e-8, 100)
    assert it <= 6 * 1 + 1 + 3 and rel <= 1e-8                # M^-1 H = identity + rank 6 L
    assert np.abs(x - xd).max() < 1e-9
    x, it, rel = R.pcg(lin, 0.0, R.make_precond("jacobi", g["init"], lin, g["Omega"], 0.0), 1e-8, 1000)
    assert 16 < it < 1000 and np.abs(x - xd).max() < 5e-9


@pytest.mark.parametrize("kind", ["jacobi", "chain"])
def test_reference_optimizer_recovers_true_poses_from_exact_measurements(kind):
    g = R.ring(16, [(15, 0)], seed=7, noise_t=0.0, noise_r=0.0)
    rng = np.random.default_rng(8)
    start = np.stack([g["true"][0]] + [R.mul_se3(T, R.exp_se3(np.array([0.1] * 3 + [0.03] * 3) * rng.standard_normal(6)))
                                       for T in g["true"][1:]])
    o = R.optimize(start, g["fixed"], g["edges"], g["Z"], g["Omega"], preconditioner=kind)
    assert o["converged"] and o["cost_final"] < 1e-16
    assert np.abs(o["poses"][:, :3, 3] - g["true"][:, :3, 3]).max() < 1e-8
    rot = max(np.linalg.norm(R.log_so3(a[:3, :3].T @ b[:3, :3])) for a, b in zip(o["poses"], g["true"]))
    assert rot < 1e-8


def test_reference_outlier_case_turns_down_the_outlier_alone():
    g = R.case("n16_outlier")
    o = R.optimize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], solver="dense")
    assert o["converged"] and o["weights"][-1] < 1.0 and np.all(o["weights"][:-1] == 1.0)


def test_incidence_list_matches_the_reference():
    from overlapnet_amd import pose_graph as PG
    rng = np.random.default_rng(9)
    e = np.array([(i, j) for i, j in rng.integers(0, 12, (40, 2)) if i != j], np.int32)
    ptr, lst = PG.incidence(12, e)
    rp, rl = R.incidence(12, e)
    assert np.array_equal(ptr, rp) and np.array_equal(lst, rl) and ptr.dtype == np.int32 and lst.dtype == np.int32


def test_python_refusals():
    from overlapnet_amd import pose_graph as PG
    poses = np.stack([np.eye(4)] * 5)
    om = PG.information_from_sigmas(0.05, 0.01)
    assert np.allclose(np.diag(om), [400.0] * 3 + [1e4] * 3)
    for bad in ((0.0, 1.0), (1.0, -1.0), (np.nan, 1.0)):
        with pytest.raises(ValueError):
            PG.information_from_sigmas(*bad)
    g = PG.PoseGraph(None, poses)
    with pytest.raises(ValueError, match="itself"):
        g.add_edge(2, 2, np.eye(4), om)
    for i, j in ((-1, 0), (0, 5)):
        with pytest.raises(ValueError, match="outside"):
            g.add_edge(i, j, np.eye(4), om)
    for bad in (np.zeros((6, 6)), -om, np.diag([1.0] * 5 + [0.0]), om + np.triu(np.ones((6, 6)), 1), np.full((6, 6), np.nan)):
        with pytest.raises(ValueError, match="positive definite"):
            g.add_edge(0, 1, np.eye(4), bad)
    with pytest.raises(ValueError, match="fixed node 7"):
        PG.PoseGraph(None, poses, fixed=(7,))
    with pytest.raises(ValueError, match="no fixed node"):
        PG.PoseGraph(None, poses, fixed=()).optimize()
    for k in range(3):
        g.add_edge(k, k + 1, np.eye(4), om)
    with pytest.raises(ValueError, match="free node 4 has no edge"):
        g.optimize()
    h = PG.PoseGraph(None, poses)
    h.add_edge(0, 1, np.eye(4), om)
    h.add_edge(2, 3, np.eye(4), om)
    h.add_edge(3, 4, np.eye(4), om)
    with pytest.raises(ValueError, match="component without a fixed node"):
        h.optimize()
    c = PG.PoseGraph(None, poses)
    c.add_odometry(poses, om)
    assert c.chain_available() and c.choose_preconditioner("chain") == "chain"
    c.add_edge(4, 0, np.eye(4), om)
    assert c.chain_available() and c.choose_preconditioner("auto") in ("chain", "jacobi")
    with pytest.raises(ValueError, match="no preconditioner"):
        c.choose_preconditioner("ilu")
    d = PG.PoseGraph(None, poses, fixed=(0, 2))
    d.add_odometry(poses, om)
    assert not d.chain_available() and d.choose_preconditioner("auto") == "jacobi"
    with pytest.raises(ValueError, match="chain preconditioner needs"):
        d.choose_preconditioner("chain")
    r = PG.PoseGraph(None, poses)                              # loop edges first: not a chain
    r.add_edge(4, 0, np.eye(4), om)
    r.add_odometry(poses, om)
    assert not r.chain_available()
    with pytest.raises(ValueError, match="verify_top_k ran without"):
        c.add_loop_closures(4, [(1, 0.9, 0, np.eye(4), 0.8, 0.02, None)], om)
    assert c.add_loop_closures(4, [(1, 0.9, 0, np.eye(4), 0.8, 0.02, True), (2, 0.5, 0, np.eye(4), 0.1, 0.5, False)], om) == 1
    assert tuple(c.edges[-1]) == (4, 1)


def test_auto_rule():
    from overlapnet_amd import pose_graph as PG
    om = PG.information_from_sigmas(0.05, 0.01)
    poses = np.stack([np.eye(4)] * 64)
    g = PG.PoseGraph(None, poses)
    g.add_odometry(poses, om)
    g.add_edge(63, 0, np.eye(4), om)
    assert g.choose_preconditioner("auto") == "chain"          # 6 + 1 < 2.9 * 64
    for k in range(29):
        g.add_edge(62 - k, k + 1, np.eye(4), om)
    assert g.choose_preconditioner("auto") == "chain"          # 6 * 30 + 1 = 181 < 185.6
    g.add_edge(30, 32, np.eye(4), om)
    assert g.choose_preconditioner("auto") == "jacobi"         # 6 * 31 + 1 = 187


def test_library_argument_errors_need_no_gpu():
    from overlapnet_amd import _lib
    lib = _lib.load()
    assert lib.ovn_pose_graph_workspace_bytes(16, 17) > 0
    assert lib.ovn_pose_graph_workspace_bytes(0, 1) == 0 and lib.ovn_pose_graph_workspace_bytes(4, -1) == 0
    assert lib.ovn_pose_graph_workspace_bytes((1 << 20) + 1, 1) == 0 and lib.ovn_pose_graph_workspace_bytes(4, (1 << 22) + 1) == 0
    assert lib.ovn_pose_graph_workspace_bytes(256, 300) >= lib.ovn_pose_graph_workspace_bytes(256, 0)
    assert lib.ovn_pose_graph_linearize(*([None] * 4), 4, None, None, None, 3, None, None, 1.0, *([None] * 11)) == 1
    assert b"ctx is NULL" in lib.ovn_last_error()
    assert lib.ovn_pose_graph_solve(None, None, None, 4, None, 3, *([None] * 7), 0, 0.0, 1e-8, 0, 1, None, None, None) == 1
    assert lib.ovn_pose_graph_precondition(None, None, 4, 0, 0.0, None, None, None, None, None) == 1
    assert lib.ovn_pose_graph_retract(None, None, None, None, None, 4, None, None, None) == 1


def test_slam_tool_has_no_default_thresholds(tmp_path):
    from overlapnet_amd import odometry
    from tools import slam
    base = ["--config", "c.json", "--scans", "s", "--out", "o.txt"]
    need = {"--overlap-thres": ["0.3"], "--min-fitness": ["none"], "--max-rms": ["0.1"], "--odom-sigma": ["0.05", "0.01"],
            "--loop-sigma": ["0.1", "0.02"], "--huber": ["None"]}
    full = base + [t for k, v in need.items() for t in [k] + v]
    a = slam.parse(full)
    assert a.overlap_thres == 0.3 and a.min_fitness is None and a.max_rms == 0.1 and a.huber is None
    assert a.odom_sigma == [0.05, 0.01] and a.loop_sigma == [0.1, 0.02] and a.preconditioner == "auto"
    for k in need:                                             # each of them is required: nothing is chosen for the user
        rest = base + [t for kk, v in need.items() if kk != k for t in [kk] + v]
        with pytest.raises(SystemExit):
            slam.parse(rest)
    with pytest.raises(SystemExit):
        slam.parse(full + ["--min-gap", "0"])
    poses = np.stack([R.exp_se3(np.random.default_rng(k).standard_normal(6)) for k in range(4)])
    path = str(tmp_path / "poses.txt")
    odometry.write_poses(path, poses)
    assert np.array_equal(slam.read_pose_lines(path), poses)
