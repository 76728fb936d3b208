"""CPU: the mathematics of the marginal covariances as tests/_pose_graph_marginals_ref.py states it, what
tests/test_gpu_pose_graph_marginals.py builds on, the refusals of `PoseGraph.marginals` and of the library before any GPU work, and
the covariance file and search ellipses of overlapnet_amd.lcd.

Measured here (NumPy fp64), relative to the largest entry of Gamma[N - 1]: the restatement against the diagonal blocks of
numpy.linalg.inv of the dense reduced Hessian 4.4e-16 .. 1.1e-14 (bound 1e-9, section 33's for its apply at the same condition
numbers); against its own reversed-sum form 3.4e-16 .. 7.3e-16; the L = 0 restatement against first-order covariance propagation
2.6e-15 (bound 1e-12)."""
import json
import os

import numpy as np
import pytest

from tests import _pose_graph_loops_ref as LR
from tests import _pose_graph_marginals_ref as MR
from tests import _pose_graph_ref as R

SMALL = sorted(R.CASES) + ["mixed"]
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pose_graph_marginals.json")


def _graph(name):
    return LR.mixed() if name == "mixed" else R.case(name)


def _lin(g, reverse=False):
    return R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], reverse=reverse)


@pytest.fixture(scope="module")
def ref():
    out = {}
    for name in SMALL:
        g = _graph(name)
        lin = _lin(g)
        out[name] = dict(g=g, lin=lin, fwd=MR.prepare(g["init"], lin, g["Omega"]),
                         rev=MR.prepare(g["init"], _lin(g, True), g["Omega"], True))
    return out


@pytest.mark.parametrize("frame", MR.FRAMES)
@pytest.mark.parametrize("name", SMALL)
def test_restatement_is_the_diagonal_of_the_dense_inverse(ref, name, frame):
    c = ref[name]
    g, n = c["g"], len(c["g"]["init"])
    got = MR.marginals(c["fwd"], g["init"], range(n), frame)
    back = MR.marginals(c["rev"], g["init"], range(n), frame, reverse=True)
    want = MR.dense_marginals(c["lin"], g["init"], frame)
    err, fig = MR.distance(got, want, c["fwd"]), MR.distance(got, back, c["fwd"])
    print("POSE_GRAPH_MARGINALS %s %s: the restatement against inv(H) %.3g, against its reversed sums %.3g (scale %.3g)"
          % (name, frame, err, fig, MR.scale(c["fwd"])))
    assert err <= 1e-9
    assert MR.distance(back, want, c["fwd"]) <= 1e-9
    # structure: node 0, symmetry to the bit, positive up to the rounding of the subtraction Gamma - Y'Y
    assert np.all(got[0] == 0.0)
    assert np.array_equal(got, np.swapaxes(got, 1, 2))
    low = min(np.linalg.eigvalsh(S).min() for S in got[1:])
    assert low >= -10.0 * fig * MR.scale(c["fwd"])


@pytest.mark.parametrize("name", SMALL)
def test_a_loop_edge_never_increases_a_trace(ref, name):
    """Sigma with one more edge is Sigma minus a positive semidefinite matrix, in either frame; what rounding can add is the
    restatement's distance from its reversed form, times ten."""
    c = ref[name]
    g, n = c["g"], len(c["g"]["init"])
    loops = len(g["edges"]) - (n - 1)
    slack = 10.0 * max(MR.distance(MR.marginals(c["fwd"], g["init"], range(n), f), MR.marginals(c["rev"], g["init"], range(n), f, True),
                                   c["fwd"]) for f in MR.FRAMES) * MR.scale(c["fwd"])
    for frame in MR.FRAMES:
        before = None
        for k in range(loops + 1):
            lin = LR.restrict(c["lin"], n - 1 + k)
            p = MR.prepare(g["init"], lin, g["Omega"][:n - 1 + k])
            tr = np.trace(MR.marginals(p, g["init"], range(n), frame), axis1=1, axis2=2)
            if before is not None:
                assert np.all(tr <= before + slack), (frame, k)
                assert np.any(tr < before) or not p["span"][k - 1, 3]
            before = tr


def test_without_loops_it_is_first_order_covariance_propagation():
    """Exact measurements (r = 0, so B = I): Sigma_{k+1} = Ad(Z_k^-1) Sigma_k Ad(Z_k^-1)' + Omega_k^-1 in the local frame."""
    rng = np.random.default_rng(12)
    n = 40
    poses = [R.exp_se3(rng.standard_normal(6))]
    Z, Om = [], []
    for k in range(n - 1):
        Z.append(R.exp_se3(rng.standard_normal(6) * np.array([1.0, 1.0, 0.3, 0.05, 0.05, 0.4])))
        poses.append(R.mul_se3(poses[-1], Z[-1]))
        A = rng.standard_normal((6, 6))
        Om.append(A @ A.T + 6.0 * np.eye(6))
    poses, Z, Om = np.stack(poses), np.stack(Z), np.stack(Om)
    edges = np.array([(k, k + 1) for k in range(n - 1)])
    fixed = np.zeros(n, bool)
    fixed[0] = True
    lin = R.linearize(poses, fixed, edges, Z, Om)
    assert np.abs(lin["r"]).max() <= 1e-12
    for reverse in (False, True):
        p = MR.prepare(poses, lin, Om, reverse)
        got = MR.marginals(p, poses, range(n), "local", reverse)
        want = np.zeros((n, 6, 6))
        for k in range(n - 1):
            Ad = R.adjoint(R.inv_se3(Z[k]))
            want[k + 1] = Ad @ want[k] @ Ad.T + np.linalg.inv(Om[k])
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print("POSE_GRAPH_MARGINALS L = 0: the restatement against first-order propagation %.3g (reversed sums: %s)" % (err, reverse))
        assert err <= 1e-12
    assert len(p["C"]) == 0 and np.array_equal(MR.world(p, [7])[0], MR.mirror(p["gamma"][7]))


def test_position_jacobian_against_central_differences():
    rng = np.random.default_rng(13)
    h = 1e-6
    for _ in range(10):
        T = R.exp_se3(rng.standard_normal(6) * np.array([20.0, 20.0, 5.0, 1.0, 1.0, 1.0]))
        J = MR.position_jacobian(T)
        num = np.zeros((6, 6))
        for q in range(6):
            e = np.zeros(6)
            e[q] = h
            Tp, Tm = R.mul_se3(R.exp_se3(e), T), R.mul_se3(R.exp_se3(-e), T)
            num[:3, q] = (Tp[:3, 3] - Tm[:3, 3]) / (2 * h)
            num[3:, q] = R.log_so3(Tp[:3, :3] @ Tm[:3, :3].T) / (2 * h)      # the rotation vector in the world
        assert np.abs(J - num).max() <= 1e-6 * np.abs(J).max()


def test_queries_in_any_order_with_repeats_and_outside_ids(ref):
    c = ref["mixed"]
    g = c["g"]
    every = MR.marginals(c["fwd"], g["init"], range(16), "position")
    ids = [15, 3, 3, 0, -1, 9, 16, 3]
    got = MR.marginals(c["fwd"], g["init"], ids, "position")
    for k, S in zip(ids, got):
        assert np.isnan(S).all() if not 0 <= k < 16 else np.array_equal(S, every[k])
    lo = int(c["fwd"]["span"][:, 0].min())
    assert lo == 0                                                    # `mixed` has a span from node 0: no node lies before every lo
    p = ref["n16_loop1"]["fwd"]
    lo = int(p["span"][0, 0])
    for k in range(lo + 1):                                           # before the span: Gamma alone
        assert np.array_equal(MR.world(p, [k])[0], MR.mirror(p["gamma"][k]))


def test_python_refusals():
    from overlapnet_amd import pose_graph as PG
    om = PG.information_from_sigmas(0.05, 0.01)
    poses = np.stack([np.eye(4)] * 64)
    d = PG.PoseGraph(None, poses, fixed=(0, 2))                      # the chain precondition fails: two fixed nodes
    d.add_odometry(poses, om)
    with pytest.raises(ValueError, match="marginal covariances need edges 0 .. N - 2"):
        d.marginals()
    r = PG.PoseGraph(None, poses)                                    # loop edges first: not a chain
    r.add_edge(4, 0, np.eye(4), om)
    r.add_odometry(poses, om)
    with pytest.raises(ValueError, match="marginal covariances need edges 0 .. N - 2"):
        r.marginals()
    big = PG.PoseGraph(None, poses)
    big.add_odometry(poses, om)
    big._ij += [(40, 3)] * (PG.MAX_LOOPS + 1)                        # past add_edge, for speed
    with pytest.raises(ValueError, match="at most %d loop edges after the chain, the graph has %d" % (PG.MAX_LOOPS, PG.MAX_LOOPS + 1)):
        big.marginals()
    c = PG.PoseGraph(None, poses)
    c.add_odometry(poses, om)
    with pytest.raises(ValueError, match="no frame"):
        c.marginals(frame="world")
    with pytest.raises(ValueError, match="huber must be > 0"):
        c.marginals(huber=0.0)
    with pytest.raises(ValueError, match="nodes must be integers in 0..63"):
        c.marginals(nodes=[3, 64])
    with pytest.raises(ValueError, match="nodes must be integers"):
        c.marginals(nodes=[0.5])
    with pytest.raises(ValueError, match="no node asked for"):
        c.marginals(nodes=[])
    with pytest.raises(ValueError, match=r"poses must be \(64,4,4\)"):
        c.marginals(poses=poses[:5])


def test_library_limits_and_argument_errors_need_no_gpu():
    import re
    from overlapnet_amd import _lib
    from overlapnet_amd import pose_graph as PG
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(HERE), "include", "ovn_hip.h")).read()
    assert re.search(r"#define OVN_POSE_GRAPH_COV_LOCAL 0\b", header) and re.search(r"#define OVN_POSE_GRAPH_COV_POSITION 1\b", header)
    kmax = 1 << int(re.search(r"#define OVN_POSE_GRAPH_MAX_QUERY \(1 << (\d+)\)", header).group(1))
    cap = PG.MAX_LOOPS
    f = lib.ovn_pose_graph_marginals_bytes
    assert f(2, 0, 1) > 0 and f(2, 1, 1) > 0 and f(1 << 20, cap, kmax) > 0
    assert f(1, 0, 1) == 0 and f((1 << 20) + 1, 0, 1) == 0 and f(16, -1, 1) == 0 and f(16, cap + 1, 1) == 0
    assert f(16, 1, 0) == 0 and f(16, 1, kmax + 1) == 0
    sp = lambda L: (6 * L + LR.BLOCK - 1) // LR.BLOCK * LR.BLOCK
    tiles = lambda K: min((K + MR.TILE - 1) // MR.TILE, MR.CHUNK // MR.TILE)
    even = lambda v: (v + 1) // 2 * 2
    for n, L, K in ((600, 0, 600), (600, 9, 1), (600, 9, 7), (600, 9, 8), (600, 9, 9), (16384, cap, 16384), (16384, cap, kmax)):
        gam = even(36 * n) + even(72 * ((n - 1 + 255) // 256)) if L == 0 else 0
        assert f(n, L, K) == 8 * (even((K + 255) // 256) + gam + even(tiles(K) * sp(L) * 48)), (n, L, K)
    assert f(1 << 20, cap, kmax) - 8 * even(kmax // 256) == 8 * 512 * sp(cap) * 48 <= 302e6     # bounded however many are asked for
    assert lib.ovn_pose_graph_marginals(None, None, None, 4, 3, 0, None, None, None, 1, 0, None, None, None) == 1
    assert b"ctx is NULL" in lib.ovn_last_error()


def test_covariance_file_round_trip_and_the_reference_parse(tmp_path, ref):
    from overlapnet_amd import lcd
    c = ref["n64_loop2"]
    cov = MR.marginals(c["fwd"], c["g"]["init"], range(64), "position")
    cov[5, 0, 0] = 1.0 / 3.0
    cov[6, 1, 2] = 1e-300
    path = str(tmp_path / "covariance.txt")
    lcd.write_covariances(path, cov)
    back = lcd.read_covariances(path)
    assert back.shape == (64, 6, 6) and np.array_equal(back.view(np.int64), cov.view(np.int64))
    # the reference's own three lines
    covs = open(path)
    covs = [overlap.replace('\n', '').split() for overlap in covs.readlines()]
    covs = np.asarray(covs, dtype=float)
    assert covs.shape == (64, 36)
    for idx in range(64):
        assert np.array_equal(covs[idx].reshape((6, 6)), cov[idx])
    ell = lcd.ellipses_from_covariances(cov, 3.0)
    assert len(ell) == 64 and all(e == lcd.covariance_ellipse(S, 3.0) for e, S in zip(ell, cov))
    assert lcd.ellipses_from_covariances(cov, 2.0)[9] == lcd.covariance_ellipse(cov[9][:2, :2], 2.0)
    with pytest.raises(ValueError):
        lcd.write_covariances(path, cov[0])
    with open(path, "a") as fh:
        fh.write("1 2 3\n")
    with pytest.raises(ValueError, match="36 numbers"):
        lcd.read_covariances(path)


def test_gate_on_a_drive_that_comes_back():
    """300 frames: 150 m out along x, back on a lane 2 m to the side.  With dead reckoning's covariance as the search space, a frame on
    the way back keeps the frames it passes and drops those farther than its ellipse."""
    from overlapnet_amd import lcd
    g = MR.GATE
    gold = json.load(open(GOLDEN))
    assert gold["geometry"] == g
    cand = MR.gate_candidates()
    assert {str(k): v for k, v in cand.items() if v} == gold["candidates"]
    d = MR.gate_drive()
    lin = _lin(d)
    cov = MR.marginals(MR.prepare(d["init"], lin, d["Omega"]), d["init"], range(g["frames"]), "position")
    ell = lcd.ellipses_from_covariances(cov, g["nstd"])
    xy = d["init"][:, :2, 3]
    checked = 0
    for k in range(g["out_frames"] + 20, g["frames"]):
        passed = 2 * g["out_frames"] - 1 - k                         # the frame this one passes at `lane` metres
        if passed > k - g["min_gap"]:
            continue
        w, h, _ = ell[k]
        assert passed in cand[k], "the ellipse reaches the other lane"
        far = [r for r in range(k - g["min_gap"] + 1) if np.linalg.norm(xy[r] - xy[k]) > max(w, h) / 2.0]
        assert far and not set(far) & set(cand[k])
        assert all(np.linalg.norm(xy[r] - xy[k]) <= max(w, h) / 2.0 for r in cand[k])
        checked += 1
    assert checked >= 50
    assert all(not cand[k] for k in range(g["min_gap"] - 1))


def test_slam_tool_offers_the_new_options():
    from tools import slam
    base = ["--config", "c.json", "--scans", "s", "--out", "o.txt", "--overlap-thres", "0.3", "--min-fitness", "none", "--max-rms", "0.1",
            "--odom-sigma", "0.05", "0.01", "--loop-sigma", "0.1", "0.02", "--huber", "None"]
    a = slam.parse(base)
    assert a.covariances is None and a.gate_sigma is None
    a = slam.parse(base + ["--covariances", "cov.txt", "--gate-sigma", "3"])
    assert a.covariances == "cov.txt" and a.gate_sigma == 3.0
    with pytest.raises(SystemExit):
        slam.parse(base + ["--gate-sigma", "0"])
