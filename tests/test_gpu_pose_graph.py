"""GPU (MI355X): the pose-graph kernels (csrc/pose_graph.hip) against their NumPy statement (tests/_pose_graph_ref.py).

Cases: rings of 16 and 64 poses (radius 4 m, odometry noise 0.02 m / 0.004 rad, Omega = diag(1 / 0.05^2 x 3, 1 / 0.01^2 x 3), node 0
fixed): n16_loop1 = one loop (15, 0); n16_outlier = loops (15, 0), (12, 1) and an outlier edge (4, 11) displaced by
Exp(3, -2, 0.5, 0, 0, 0.7) at huber 1.5; n64_loop2 = loops (63, 0), (40, 3).

Tolerances.  Both sides are fp64 and differ in libm and in nothing else that is known: the kernel takes the reference's sums in the
reference's order.  The allowance is measured on the reference itself:
  LIN_FIGURE  the reference's linearization against itself with every sum reversed: r, s, w, g, the diagonal blocks and the cost
              differ by at most 5.4e-15 of the quantity's largest magnitude (5.4e-15, 2.7e-15, 5.8e-16 on the three cases); rounded
              up to 6e-15.  LIN_TOL = ten times that, 6e-14, relative to the largest magnitude of the quantity compared.
  PCG         after k = 5 iterations the reversed reference PCG is within 3.5e-15 of the forward one (relative to |delta|_inf), inside
              LIN_TOL * k, which is the bound used.  At convergence (rtol 1e-8) the reference PCG leaves against numpy.linalg.solve
              |delta - delta_dense|_inf = 2.9e-10 / 7.1e-10 / 3.1e-9 (block-Jacobi) and 7.3e-15 / 1.6e-9 / 2.3e-9 (chain) on the three
              cases, and numpy.linalg.solve itself moves by 2e-15 when the system is permuted; the GPU is allowed ten times the sum.
  OPT_FIGURE  the reference optimizer run with its own PCG (either preconditioner) ends at most 1.37e-9 (largest pose entry) from the
              reference run with a dense solve; rounded up to 1.4e-9, the GPU is allowed ten times that against the dense reference.
  SCAN        the chain preconditioner by numpy.cumsum against the same sums in the kernel's order (Hillis-Steele in blocks of 256,
              block totals in order): measured per shape inside the test, the GPU is allowed ten times that figure.
Rotation drift: nothing is re-orthonormalized; a retraction multiplies two rotations (error a few eps per entry), so after at most 30
outer iterations |R'R - I| stays below 30 * 16 eps = 1.1e-13, which the optimize tests hold."""
import numpy as np
import pytest
import torch

from tests import _pose_graph_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

LIN_FIGURE = 6e-15
LIN_TOL = 10 * LIN_FIGURE
PCG_LEAVES = {("n16_loop1", "jacobi"): 2.9e-10, ("n16_outlier", "jacobi"): 7.1e-10, ("n64_loop2", "jacobi"): 3.1e-9,
              ("n16_loop1", "chain"): 7.3e-15, ("n16_outlier", "chain"): 1.6e-9, ("n64_loop2", "chain"): 2.3e-9}
DENSE_SELF = 2e-15
OPT_FIGURE = 1.4e-9
DRIFT = 30 * 16 * np.finfo(np.float64).eps
NAMES = sorted(R.CASES)
KINDS = ("jacobi", "chain")


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    e = OvnEngine(64, 900, 1, device=0)
    yield e
    torch.cuda.synchronize()
    e.close()


def _up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _graph(eng, g, chain=True, poses=None):
    """The graph on the device: the inputs of the engine calls and their buffers."""
    n, e = len(g["init"]), len(g["edges"])
    ptr, lst = R.incidence(n, g["edges"])
    return dict(poses=_up(eng, g["init"] if poses is None else poses), fixed=_up(eng, g["fixed"].astype(np.uint8)),
                ij=_up(eng, g["edges"].astype(np.int32).reshape(e, 2)), meas=_up(eng, g["Z"].reshape(e, 4, 4)),
                info=_up(eng, g["Omega"].reshape(e, 6, 6)), ptr=_up(eng, ptr), lst=_up(eng, lst), huber=g["huber"],
                buf=eng.pose_graph_buffers(n, e, chain=chain))


def _linearize(eng, d, **kw):
    return eng.pose_graph_linearize(d["poses"], d["fixed"], d["ij"], d["meas"], d["info"], d["ptr"], d["lst"], d["huber"], d["buf"],
                                    **kw).cpu().numpy()


def _solve(eng, d, kind, lam=0.0, rtol=1e-8, first=0, iters=32):
    return eng.pose_graph_solve(d["fixed"], d["ij"], d["ptr"], d["lst"], d["buf"], kind, lam, rtol, first, iters).cpu().numpy()


def _solve_to_convergence(eng, d, kind, lam=0.0, rtol=1e-8, chunk=32, cap=2000):
    done = 0
    while True:
        rec = _solve(eng, d, kind, lam, rtol, done, chunk)
        done += chunk
        if rec[6] or rec[7] or done >= cap:
            return rec


def _rel(a, b):
    """|a - b|_inf relative to the largest magnitude of b."""
    b = np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (scale if scale > 0 else 1.0))


@pytest.fixture(scope="module")
def ref():
    """Per case: the graph, the reference linearization at the start (forward and with reversed sums), the dense solution."""
    out = {}
    for name in NAMES:
        g = R.case(name)
        lin = R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"])
        rev = R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], reverse=True)
        out[name] = dict(g=g, lin=lin, rev=rev, dense=R.dense_solve(lin, 0.0))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_linearization(eng, ref, name):
    c = ref[name]
    g, lin, rev = c["g"], c["lin"], c["rev"]
    fig = max(_rel(rev[k], lin[k]) for k in ("r", "s", "w", "g", "D"))
    fig = max(fig, abs(rev["cost"] - lin["cost"]) / lin["cost"])
    print("POSE_GRAPH %s: the reference against itself with reversed sums %.3g (LIN_FIGURE %.3g)" % (name, fig, LIN_FIGURE))
    assert fig <= LIN_FIGURE, "the figure in this file's docstring no longer covers the reference"
    d = _graph(eng, g)
    rec = _linearize(eng, d)
    b = {k: v.cpu().numpy() for k, v in d["buf"].items()}
    got = dict(r=b["res"], s=b["chi"], w=b["weight"], g=b["grad"], D=b["diag"], A=b["jac"][:, 0], B=b["jac"][:, 1], Hii=b["blocks"][:, 0],
               Hij=b["blocks"][:, 1], Hjj=b["blocks"][:, 2])
    for k, v in got.items():
        err = _rel(v, lin[k])
        print("POSE_GRAPH %s: %-3s differs by %.3g of its largest magnitude" % (name, k, err))
    for k, v in got.items():
        assert _rel(v, lin[k]) <= LIN_TOL, k
    assert abs(rec[0] - lin["cost"]) <= LIN_TOL * lin["cost"]
    assert rec[1] == 0 and rec[2] == 0
    assert abs(rec[3] - np.abs(lin["g"]).max()) <= LIN_TOL * np.abs(lin["g"]).max()
    free = np.flatnonzero(~g["fixed"])
    eye = np.einsum("nab,nbc->nac", b["diag"][free], b["dinv"][free])
    assert np.abs(eye - np.eye(6)).max() < 1e-9                     # cond of a diagonal block is about 1e4
    assert np.all(b["dinv"][g["fixed"]] == 0) and np.all(b["grad"][g["fixed"]] == 0)
    G, N = R.chain_terms(g["init"], lin, g["Omega"])
    assert _rel(b["chain"][:, 1], N) <= LIN_TOL
    assert _rel(b["chain"][:, 0], G) <= 1e-9                        # through two inverses: B^-1 and (w Omega)^-1
    # the cost-only call: the same residuals, weights and cost, nothing else written
    d["buf"]["grad"].fill_(7.0)
    rec2 = torch.zeros(16, dtype=torch.float64, device=eng.device)
    _linearize(eng, d, jacobians=False, record=rec2)
    assert rec2.cpu().numpy()[0] == rec[0] and np.all(d["buf"]["grad"].cpu().numpy() == 7.0)
    assert np.array_equal(d["buf"]["res"].cpu().numpy(), b["res"]) and np.array_equal(d["buf"]["weight"].cpu().numpy(), b["weight"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_solve_after_the_same_iterations(eng, ref, name, kind):
    c, k = ref[name], 5
    g, lin = c["g"], c["lin"]
    want, it, _ = R.pcg(lin, 0.0, R.make_precond(kind, g["init"], lin, g["Omega"], 0.0, scan=True), 0.0, k)
    assert it == k
    d = _graph(eng, g)
    _linearize(eng, d)
    rec = _solve(eng, d, kind, rtol=0.0, iters=k)
    got = d["buf"]["delta"].cpu().numpy()
    print("POSE_GRAPH %s %s: delta after %d iterations differs by %.3g of |delta|_inf (bound %.3g), record %s"
          % (name, kind, k, _rel(got, want), LIN_TOL * k, rec[4:8]))
    assert rec[4] == k and rec[6] == 0 and rec[7] == 0
    assert np.all(got[g["fixed"]] == 0)
    assert _rel(got, want) <= LIN_TOL * k


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_solve_at_convergence(eng, ref, name, kind):
    c = ref[name]
    g = c["g"]
    d = _graph(eng, g)
    _linearize(eng, d)
    rec = _solve_to_convergence(eng, d, kind)
    got = d["buf"]["delta"].cpu().numpy()
    err, bound = float(np.abs(got - c["dense"]).max()), 10 * (PCG_LEAVES[(name, kind)] + DENSE_SELF)
    print("POSE_GRAPH %s %s: converged after %d iterations at %.3g, |delta - dense|_inf %.3g (bound %.3g)" % (name, kind, rec[4], rec[5], err, bound))
    assert rec[6] == 1 and rec[7] == 0 and rec[5] <= 1e-8
    assert np.isfinite(got).all()
    if (name, kind) == ("n16_loop1", "chain"):
        assert rec[4] <= 6 * 1 + 1 + 3                              # M^-1 H = identity + rank 6 L; 3 iterations for fp64 rounding
    assert err <= bound
    # launches enqueued after convergence leave everything as it is
    again = _solve(eng, d, kind, first=int(rec[4]) + 64, iters=8)
    assert np.array_equal(again, rec) and np.array_equal(d["buf"]["delta"].cpu().numpy(), got)


def _optimize(eng, g, **kw):
    from overlapnet_amd.pose_graph import PoseGraph
    pg = PoseGraph(eng, g["init"], fixed=np.flatnonzero(g["fixed"]))
    for (i, j), Z, om in zip(g["edges"], g["Z"], g["Omega"]):
        pg.add_edge(i, j, Z, om)
    return pg, pg.optimize(huber=None if np.isinf(g["huber"]) else g["huber"], **kw)


def _grad_max(eng, g, poses):
    return _linearize(eng, _graph(eng, g, poses=poses))[3]


@pytest.mark.parametrize("kind", KINDS + ("auto",))
@pytest.mark.parametrize("name", NAMES)
def test_optimize(eng, ref, name, kind):
    g = ref[name]["g"]
    want = R.optimize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], max_iterations=30, solver="dense")
    assert want["converged"]
    pg, res = _optimize(eng, g, preconditioner=kind)
    err = float(np.abs(res.poses - want["poses"]).max())
    g0, g1 = np.abs(ref[name]["lin"]["g"]).max(), _grad_max(eng, g, res.poses)
    drift = max(np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() for T in res.poses)
    print("POSE_GRAPH %s %s (%s): %d outer / %d PCG iterations, cost %.10g -> %.10g (reference %.10g in %d), poses within %.3g (bound "
          "%.3g), |g|_inf %.3g -> %.3g, |R'R - I| %.3g" % (name, kind, pg.choose_preconditioner(kind), res.outer_iterations,
                                                          res.cg_iterations, res.cost_initial, res.cost_final, want["cost_final"],
                                                          want["outer_iterations"], err, 10 * OPT_FIGURE, g0, g1, drift))
    assert res.converged and res.outer_iterations <= 30
    assert err <= 10 * OPT_FIGURE
    assert abs(res.cost_final - want["cost_final"]) <= 1e-9 * want["cost_final"]
    assert g1 < 1e-6 * g0
    assert drift <= DRIFT
    assert np.array_equal(res.poses[0], g["init"][0])
    assert res.chi2.shape == res.weights.shape == (len(g["edges"]),)
    assert np.abs(res.chi2 - want["chi2"]).max() <= 1e-6 * want["chi2"].max()
    if name == "n16_outlier":
        assert res.weights[-1] < 1.0 and np.all(res.weights[:-1] == 1.0)
        assert abs(res.weights[-1] - want["weights"][-1]) <= 1e-8
    else:
        assert np.all(res.weights == 1.0)


@pytest.mark.parametrize("kind", KINDS)
def test_exact_measurements_give_the_true_poses_back(eng, kind):
    g = R.ring(16, [(15, 0)], seed=7, noise_t=0.0, noise_r=0.0)
    rng = np.random.default_rng(8)
    g["init"] = np.stack([g["true"][0]] + [R.mul_se3(T, R.exp_se3(np.array([0.1] * 3 + [0.03] * 3) * rng.standard_normal(6)))
                                           for T in g["true"][1:]])
    g["huber"] = np.inf
    _, res = _optimize(eng, g, preconditioner=kind)
    dt = float(np.abs(res.poses[:, :3, 3] - g["true"][:, :3, 3]).max())
    dr = max(np.linalg.norm(R.log_so3(a[:3, :3].T @ b[:3, :3])) for a, b in zip(res.poses, g["true"]))
    print("POSE_GRAPH exact %s: %d outer iterations, cost %.3g, %.3g m and %.3g rad from the truth" % (kind, res.outer_iterations, res.cost_final, dt, dr))
    assert res.converged and dt < 1e-8 and dr < 1e-8


@pytest.mark.parametrize("n", [255, 256, 257, 512, 513, 256 * 256 + 1])
def test_chain_preconditioner_alone_across_scan_blocks(eng, n):
    """n chain edges around one and two block boundaries of the scan (256), and one more than 256 blocks."""
    rng = np.random.default_rng(n)
    G, N = rng.standard_normal((n, 6, 6)), rng.standard_normal((n, 6, 6))
    y = rng.standard_normal((n + 1, 6))
    want, order = R.chain_apply(G, N, y), R.chain_apply_scan(G, N, y)
    fig = _rel(order, want)
    buf = eng.pose_graph_buffers(n + 1, 0, chain=True)
    buf["chain"].copy_(_up(eng, np.stack([G, N], 1)))
    out = torch.full((n + 1, 6), 7.0, dtype=torch.float64, device=eng.device)
    got = eng.pose_graph_precondition(_up(eng, y), buf, "chain", out=out).cpu().numpy()
    print("POSE_GRAPH scan n = %d: cumsum against the kernel's order %.3g, the GPU against cumsum %.3g, GPU == kernel's order: %s"
          % (n, fig, _rel(got, want), np.array_equal(got, order)))
    assert np.all(got[0] == 0.0)
    assert _rel(got, want) <= 10 * fig
    assert np.array_equal(got, order), "random blocks and no libm: the scans' order of additions gives the kernels' bits"


def test_jacobi_preconditioner_alone(eng, ref):
    c = ref["n16_loop1"]
    d = _graph(eng, c["g"])
    _linearize(eng, d)
    y = np.random.default_rng(1).standard_normal((16, 6))
    got = eng.pose_graph_precondition(_up(eng, y), d["buf"], "jacobi", lam=0.5).cpu().numpy()
    want = np.einsum("nab,nb->na", R.jacobi_blocks(c["lin"]), y) / 1.5
    assert _rel(got, want) <= 1e-10 and np.all(got[0] == 0.0)


def test_same_arguments_same_bits(eng, ref):
    g = ref["n64_loop2"]["g"]
    runs = []
    for _ in range(2):
        d = _graph(eng, g)
        rec = [_linearize(eng, d).copy()]
        lin_out = {k: d["buf"][k].cpu().numpy().copy() for k in ("res", "chi", "weight", "jac", "blocks", "grad", "diag", "dinv", "chain")}
        outs = []
        for kind in KINDS:
            rec.append(_solve(eng, d, kind, rtol=0.0, iters=7).copy())
            rec.append(_solve(eng, d, kind, rtol=0.0, first=7, iters=6).copy())
            outs.append(d["buf"]["delta"].cpu().numpy().copy())
            outs.append(eng.pose_graph_precondition(d["buf"]["grad"], d["buf"], kind).cpu().numpy())
        outs.append(eng.pose_graph_retract(d["poses"], d["fixed"], d["buf"]).cpu().numpy())
        rec.append(d["buf"]["record"].cpu().numpy().copy())
        runs.append((rec, lin_out, outs))
    a, b = runs
    bits = lambda x: np.ascontiguousarray(x).view(np.int64)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(bits(x), bits(y))
    for k in a[1]:
        assert np.array_equal(bits(a[1][k]), bits(b[1][k])), k
    for x, y in zip(a[2], b[2]):
        assert np.array_equal(bits(x), bits(y))
    # 7 + 6 iterations in two chunks are 13 in one
    d = _graph(eng, g)
    _linearize(eng, d)
    one = _solve(eng, d, "chain", rtol=0.0, iters=13)
    assert one[4] == 13 and np.array_equal(bits(d["buf"]["delta"].cpu().numpy()), bits(a[2][2]))


def test_retract_matches_the_reference(eng, ref):
    g = ref["n16_loop1"]["g"]
    d = _graph(eng, g)
    delta = np.random.default_rng(2).standard_normal((16, 6)) * np.array([1.0] * 3 + [0.5] * 3)
    delta[3, 3:] *= 1e-3                                             # one node below the series switch-over
    delta[5] = 0.0
    d["buf"]["delta"].copy_(_up(eng, delta))
    got = eng.pose_graph_retract(d["poses"], d["fixed"], d["buf"]).cpu().numpy()
    want = R.retract(g["init"], delta)
    want[0] = g["init"][0]                                           # the fixed node
    assert _rel(got, want) <= LIN_TOL
    assert np.array_equal(got[0], g["init"][0]) and np.array_equal(got[5, :3], want[5, :3])
    assert d["buf"]["record"].cpu().numpy()[12] == np.abs(delta[1:]).max()


def test_second_fixed_node(eng, ref):
    from overlapnet_amd.pose_graph import PoseGraph
    g = dict(ref["n16_loop1"]["g"])
    g["fixed"] = g["fixed"].copy()
    g["fixed"][8] = True
    want = R.optimize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], max_iterations=30, solver="dense")
    pg, res = _optimize(eng, g, preconditioner="jacobi")
    assert res.converged
    assert np.array_equal(res.poses[8], g["init"][8]) and np.array_equal(res.poses[0], g["init"][0])
    assert np.abs(res.poses - want["poses"]).max() <= 10 * OPT_FIGURE
    assert pg.choose_preconditioner("auto") == "jacobi"
    with pytest.raises(ValueError, match="chain preconditioner needs"):
        pg.optimize(preconditioner="chain")
    assert isinstance(pg, PoseGraph)


def test_duplicated_edge(eng, ref):
    g = dict(ref["n16_loop1"]["g"])
    g["edges"] = np.concatenate([g["edges"], g["edges"][-1:]])
    g["Z"] = np.concatenate([g["Z"], g["Z"][-1:]])
    g["Omega"] = np.concatenate([g["Omega"], g["Omega"][-1:]])
    want = R.optimize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"], max_iterations=30, solver="dense")
    for kind in KINDS:
        _, res = _optimize(eng, g, preconditioner=kind)
        assert res.converged and np.abs(res.poses - want["poses"]).max() <= 10 * OPT_FIGURE


def test_no_edges_is_a_no_op(eng):
    n = 5
    buf = eng.pose_graph_buffers(n, 0)
    buf["delta"].fill_(7.0)
    buf["record"].fill_(3.0)
    poses = _up(eng, np.stack([np.eye(4)] * n))
    fixed = torch.zeros(n, dtype=torch.uint8, device=eng.device)
    empty = lambda *s: torch.zeros(s, dtype=torch.float64, device=eng.device)
    ij = torch.zeros((0, 2), dtype=torch.int32, device=eng.device)
    ptr, lst = torch.zeros(n + 1, dtype=torch.int32, device=eng.device), torch.zeros(0, dtype=torch.int32, device=eng.device)
    rec = eng.pose_graph_linearize(poses, fixed, ij, empty(0, 4, 4), empty(0, 6, 6), ptr, lst, 1.0, buf).cpu().numpy()
    assert np.all(rec[:4] == 0)
    rec = eng.pose_graph_solve(fixed, ij, ptr, lst, buf, "jacobi").cpu().numpy()
    assert rec[4] == 0 and rec[6] == 1 and rec[7] == 0
    assert np.all(buf["delta"].cpu().numpy() == 7.0)


def test_a_nan_measurement_is_weighted_out_and_counted(eng, ref):
    c = ref["n16_outlier"]
    g = dict(c["g"])
    g["Z"] = g["Z"].copy()
    g["Z"][-1, 1, 2] = np.nan                                        # the outlier edge (4, 11)
    d = _graph(eng, g)
    rec = _linearize(eng, d)
    b = {k: v.cpu().numpy() for k, v in d["buf"].items()}
    assert rec[1] == 1 and rec[2] == 0
    assert b["weight"][-1] == 0 and b["chi"][-1] == 0 and np.all(b["res"][-1] == 0) and np.all(b["blocks"][-1] == 0)
    assert np.all(b["weight"][:-1] > 0)
    for k in ("res", "chi", "weight", "jac", "blocks", "grad", "diag", "dinv", "chain"):
        assert np.isfinite(b[k]).all(), k
    keep = np.arange(len(g["edges"]) - 1)                            # the graph without that edge
    want = R.linearize(g["init"], g["fixed"], g["edges"][keep], g["Z"][keep], g["Omega"][keep], g["huber"])
    assert _rel(b["grad"], want["g"]) <= LIN_TOL and abs(rec[0] - want["cost"]) <= LIN_TOL * want["cost"]
    rec = _solve_to_convergence(eng, d, "jacobi")
    assert rec[6] == 1 and np.isfinite(d["buf"]["delta"].cpu().numpy()).all()
    poses = g["init"].copy()
    poses[7, 0, 3] = np.inf                                          # a non-finite pose: both of its edges
    rec = _linearize(eng, _graph(eng, c["g"], poses=poses))
    assert rec[1] == 2


def test_zero_information_breaks_down_without_touching_delta(eng, ref):
    g = dict(ref["n16_loop1"]["g"])
    g["Omega"] = np.zeros_like(g["Omega"])
    d = _graph(eng, g)
    rec = _linearize(eng, d)
    assert rec[2] > 0 and rec[0] == 0
    assert np.isfinite(d["buf"]["dinv"].cpu().numpy()).all()
    for kind in KINDS:
        d["buf"]["delta"].fill_(7.0)
        rec = _solve(eng, d, kind, iters=4)
        assert rec[7] == 1 and rec[6] == 0 and rec[4] == 0
        assert np.all(d["buf"]["delta"].cpu().numpy() == 7.0)
    from overlapnet_amd._lib import OvnError
    from overlapnet_amd.pose_graph import PoseGraph
    pg = PoseGraph(eng, g["init"])
    pg._ij, pg._z, pg._info = [tuple(e) for e in g["edges"]], list(g["Z"]), list(g["Omega"])     # past add_edge's refusal
    with pytest.raises(OvnError, match="not positive definite"):
        pg.optimize(preconditioner="jacobi")


def test_argument_errors(eng, ref):
    g = ref["n16_loop1"]["g"]
    d = _graph(eng, g)
    _linearize(eng, d)
    lib, h, s = eng.lib, eng._h, eng._stream()
    p = lambda t: None if t is None else t.data_ptr()
    b = d["buf"]
    n, e = 16, len(g["edges"])
    before = {k: v.clone() for k, v in b.items()}

    def lin(**kw):
        a = dict(poses=p(d["poses"]), fixed=p(d["fixed"]), n=n, ij=p(d["ij"]), meas=p(d["meas"]), info=p(d["info"]), e=e, ptr=p(d["ptr"]),
                 lst=p(d["lst"]), huber=1.5, res=p(b["res"]), chi=p(b["chi"]), weight=p(b["weight"]), jac=p(b["jac"]), blocks=p(b["blocks"]),
                 grad=p(b["grad"]), diag=p(b["diag"]), dinv=p(b["dinv"]), chain=p(b["chain"]), ws=p(b["ws"]), rec=p(b["record"]))
        a.update(kw)
        return lib.ovn_pose_graph_linearize(h, s, a["poses"], a["fixed"], a["n"], a["ij"], a["meas"], a["info"], a["e"], a["ptr"], a["lst"],
                                            a["huber"], a["res"], a["chi"], a["weight"], a["jac"], a["blocks"], a["grad"], a["diag"],
                                            a["dinv"], a["chain"], a["ws"], a["rec"])

    def solve(**kw):
        a = dict(fixed=p(d["fixed"]), n=n, ij=p(d["ij"]), e=e, ptr=p(d["ptr"]), lst=p(d["lst"]), blocks=p(b["blocks"]), grad=p(b["grad"]),
                 diag=p(b["diag"]), dinv=p(b["dinv"]), chain=p(b["chain"]), kind=0, lam=0.0, rtol=1e-8, first=0, iters=4,
                 delta=p(b["delta"]), ws=p(b["ws"]), rec=p(b["record"]))
        a.update(kw)
        return lib.ovn_pose_graph_solve(h, s, a["fixed"], a["n"], a["ij"], a["e"], a["ptr"], a["lst"], a["blocks"], a["grad"], a["diag"],
                                        a["dinv"], a["chain"], a["kind"], a["lam"], a["rtol"], a["first"], a["iters"], a["delta"], a["ws"],
                                        a["rec"])

    bad_lin = [dict(n=0), dict(e=-1), dict(n=(1 << 20) + 1), dict(e=(1 << 22) + 1), dict(huber=0.0), dict(huber=-1.0),
               dict(huber=float("nan")), dict(rec=None), dict(ws=None), dict(poses=None), dict(fixed=None), dict(ij=None), dict(meas=None),
               dict(info=None), dict(res=None), dict(chi=None), dict(weight=None), dict(ptr=None), dict(lst=None), dict(blocks=None),
               dict(grad=None), dict(diag=None), dict(dinv=None), dict(jac=None), dict(jac=None, blocks=None, grad=None, diag=None, dinv=None)]
    for kw in bad_lin:
        assert lin(**kw) == 1, kw
        assert lib.ovn_last_error()
    bad_solve = [dict(n=0), dict(e=-1), dict(n=(1 << 20) + 1), dict(e=(1 << 22) + 1), dict(kind=2), dict(kind=-1), dict(lam=-1e-3),
                 dict(lam=float("inf")), dict(lam=float("nan")), dict(rtol=-1.0), dict(rtol=float("nan")), dict(first=-1), dict(iters=-1),
                 dict(iters=4097), dict(rec=None), dict(ws=None), dict(delta=None), dict(fixed=None), dict(ij=None), dict(ptr=None),
                 dict(lst=None), dict(blocks=None), dict(grad=None), dict(diag=None), dict(dinv=None), dict(kind=1, chain=None)]
    for kw in bad_solve:
        assert solve(**kw) == 1, kw
    vec = p(b["grad"])
    pre = lambda n_=n, kind=0, lam=0.0, dinv=p(b["dinv"]), chain=p(b["chain"]), i=vec, o=p(b["delta"]), ws=p(b["ws"]): \
        lib.ovn_pose_graph_precondition(h, s, n_, kind, lam, dinv, chain, i, o, ws)
    for kw in (dict(n_=0), dict(n_=(1 << 20) + 1), dict(kind=3), dict(lam=-1.0), dict(lam=float("nan")), dict(dinv=None),
               dict(kind=1, chain=None), dict(i=None), dict(o=None), dict(ws=None)):
        assert pre(**kw) == 1, kw
    out = torch.empty_like(d["poses"])
    ret = lambda poses=p(d["poses"]), fixed=p(d["fixed"]), delta=p(b["delta"]), n_=n, o=p(out), ws=p(b["ws"]), rec=p(b["record"]): \
        lib.ovn_pose_graph_retract(h, s, poses, fixed, delta, n_, o, ws, rec)
    for kw in (dict(n_=0), dict(n_=(1 << 20) + 1), dict(poses=None), dict(fixed=None), dict(delta=None), dict(o=None), dict(ws=None),
               dict(rec=None)):
        assert ret(**kw) == 1, kw
    torch.cuda.synchronize()
    for k, v in b.items():
        assert torch.equal(v.view(torch.int64), before[k].view(torch.int64)), "a refused call wrote %s" % k
    assert lin() == 0 and solve() == 0 and pre() == 0 and ret() == 0
    torch.cuda.synchronize()
