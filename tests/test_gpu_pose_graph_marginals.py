"""GPU (MI355X): marginal pose covariances (ovn_pose_graph_marginals, csrc/pose_graph.hip) against their NumPy
statement (tests/_pose_graph_marginals_ref.py).

Graphs: those of tests/test_gpu_pose_graph_loops.py -- the three cases of tests/_pose_graph_ref.py, `mixed`, and the two-lap ring of
600 poses with L = 7, 8, 9, 17 (6 L = 42, 48, 54, 102: under, on and over one factor block, and two blocks plus six), whose spans cross
the scans' block boundaries at 256 and 512 -- and `chain16`, the 16-pose ring without its loop edge (L = 0).

Queries per graph: all nodes; one node; an unsorted list with repeats; 7, 8 and 9 nodes (one under, on and over the kernel's tile of 8);
the nodes up to the smallest lo (Sigma_world = Gamma[k] exactly); the nodes from the largest hi on.

Tolerance: ten times the restatement's distance from its own form with every sum reversed, relative to the largest entry of
Gamma[N - 1] (the subtraction Gamma - Y'Y cancels strongly at nodes near a closure, so the scale is Gamma and not the result); where
that distance is 0 the GPU has to agree to the bit.  Both figures are printed per graph and frame."""
import numpy as np
import pytest
import torch

from tests import _pose_graph_loops_ref as LR
from tests import _pose_graph_marginals_ref as MR
from tests import _pose_graph_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

SMALL = sorted(R.CASES) + ["mixed"]
NAMES = ["chain16"] + SMALL + ["two_lap_L%d" % L for L in LR.TWO_LAP_LOOPS]


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    torch.cuda.set_device(0)
    e = OvnEngine(64, 900, 1, device=0)
    yield e
    torch.cuda.synchronize()
    e.close()


def _lin(g):
    return R.linearize(g["init"], g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"])


def _cut(g, loops):
    e = len(g["init"]) - 1 + loops
    out = dict(g)
    out.update(edges=g["edges"][:e], Z=g["Z"][:e], Omega=g["Omega"][:e])
    return out


@pytest.fixture(scope="module")
def ref():
    """Per graph: the graph, its reference linearization, the restated prepare forward and with reversed sums, and per frame the
    restated marginals of ALL nodes in both forms (a query's expectation is a selection of rows: every column of the sweep stands alone)."""
    gs = LR.graphs()
    gs["chain16"] = _cut(R.case("n16_loop1"), 0)
    big_lin = _lin(LR.two_lap())
    out = {}
    for name, g in gs.items():
        lin = LR.restrict(big_lin, len(g["edges"])) if name.startswith("two_lap") else _lin(g)
        n = len(g["init"])
        fwd, rev = MR.prepare(g["init"], lin, g["Omega"]), MR.prepare(g["init"], lin, g["Omega"], True)
        c = dict(g=g, lin=lin, fwd=fwd, rev=rev, n=n, loops=len(g["edges"]) - (n - 1))
        for f in MR.FRAMES:
            c[f] = MR.marginals(fwd, g["init"], range(n), f)
            c[f + "_fig"] = MR.distance(MR.marginals(rev, g["init"], range(n), f, True), c[f], fwd)
        out[name] = c
    return out


def _up(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _graph(eng, g):
    n, e = len(g["init"]), len(g["edges"])
    ptr, lst = R.incidence(n, g["edges"])
    return dict(poses=_up(eng, g["init"]), fixed=_up(eng, g["fixed"].astype(np.uint8)), ij=_up(eng, g["edges"].astype(np.int32).reshape(e, 2)),
                meas=_up(eng, g["Z"].reshape(e, 4, 4)), info=_up(eng, g["Omega"].reshape(e, 6, 6)), ptr=_up(eng, ptr), lst=_up(eng, lst),
                huber=g["huber"], n=n, e=e, loops=e - (n - 1), buf=eng.pose_graph_buffers(n, e, chain=True, loops=e - (n - 1)))


def _prepare(eng, d):
    rec = eng.pose_graph_linearize(d["poses"], d["fixed"], d["ij"], d["meas"], d["info"], d["ptr"], d["lst"], d["huber"], d["buf"])
    if d["loops"] > 0:
        rec = eng.pose_graph_loops_prepare(d["poses"], d["ij"], d["info"], d["buf"])
    return rec.cpu().numpy()


def _marg(eng, d, ids, frame, **kw):
    return eng.pose_graph_marginals(d["poses"], d["buf"], _up(eng, np.asarray(ids, np.int32)), d["loops"], frame=frame, **kw).cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def _queries(c):
    n, span = c["n"], c["fwd"]["span"]
    live = span[span[:, 3] != 0] if len(span) else span
    lo = int(live[:, 0].min()) if len(live) else n - 1
    hi = int(live[:, 1].max()) if len(live) else 0
    perm = np.random.default_rng(n).permutation(n)
    q = {"all": np.arange(n), "one": [n // 2], "unsorted": [n - 1, 3, 3, 0, 7, n - 1, 5, 3, 1, n - 2, 7],
         "before": np.arange(lo + 1), "after": np.arange(hi, n)}
    for k in (MR.TILE - 1, MR.TILE, MR.TILE + 1):
        q["tile%+d" % (k - MR.TILE)] = perm[:k]
    return q, lo


@pytest.mark.parametrize("name", NAMES)
def test_parity(eng, ref, name):
    c = ref[name]
    d = _graph(eng, c["g"])
    rec = _prepare(eng, d)
    assert rec[2] == 0 and rec[13] == 0 and rec[14] == 0
    queries, lo = _queries(c)
    for frame in MR.FRAMES:
        want, fig, worst, same = c[frame], c[frame + "_fig"], 0.0, True
        for key, ids in queries.items():
            got = _marg(eng, d, ids, frame)
            r = d["buf"]["record"].cpu().numpy()
            assert r[7] == 0 and r[15] == 0
            assert np.array_equal(_bits(got), _bits(np.swapaxes(got, 1, 2))), "every block is symmetric to the bit"
            err = MR.distance(got, want[np.asarray(ids)], c["fwd"])
            worst, same = max(worst, err), same and np.array_equal(got, want[np.asarray(ids)])
            assert err <= 10 * fig, (frame, key, err, fig)
            for k, S in zip(ids, got):
                if k == 0:
                    assert np.all(S == 0.0)
        print("POSE_GRAPH_MARGINALS %s %s: the restatement against its reversed sums %.3g, the GPU against the restatement %.3g%s "
              "(scale %.3g)" % (name, frame, fig, worst, " (the same bits)" if same else "", MR.scale(c["fwd"])))
    # before every span: Gamma alone, exactly -- what the graph without its loop edges gives
    if c["loops"] > 0:
        chain = _graph(eng, _cut(c["g"], 0))
        _prepare(eng, chain)
        ids = queries["before"]
        for frame in MR.FRAMES:
            assert np.array_equal(_bits(_marg(eng, d, ids, frame)), _bits(_marg(eng, chain, ids, frame))), (frame, lo)
    if name in SMALL:                                                 # and it IS the inverse's diagonal
        for frame in MR.FRAMES:
            assert MR.distance(_marg(eng, d, np.arange(c["n"]), frame), MR.dense_marginals(c["lin"], c["g"]["init"], frame), c["fwd"]) <= 1e-9


def test_same_arguments_same_bits_and_a_chunked_query(eng, ref):
    c = ref["two_lap_L9"]
    d = _graph(eng, c["g"])
    _prepare(eng, d)
    n = c["n"]
    every = {f: _marg(eng, d, np.arange(n), f) for f in MR.FRAMES}
    for f in MR.FRAMES:
        assert np.array_equal(_bits(every[f]), _bits(_marg(eng, d, np.arange(n), f)))
    # more queries than one launch of the sweep takes: the second launch reuses the first one's tiles of the workspace
    ids = np.resize(np.random.default_rng(1).permutation(n), MR.CHUNK + 13)
    assert eng.pose_graph_marginals_bytes(n, 9, len(ids)) - eng.pose_graph_marginals_bytes(n, 9, MR.CHUNK) <= 8 * 2
    for f in MR.FRAMES:
        whole = _marg(eng, d, ids, f)
        parts = np.concatenate([_marg(eng, d, ids[:MR.CHUNK], f), _marg(eng, d, ids[MR.CHUNK:], f)])
        assert np.array_equal(_bits(whole), _bits(parts)) and np.array_equal(_bits(whole), _bits(every[f][ids]))


def test_a_nan_loop_measurement_is_left_out_and_counted(eng, ref):
    g = dict(ref["n16_outlier"]["g"])
    g["Z"] = g["Z"].copy()
    g["Z"][-1, 1, 2] = np.nan                                        # the outlier edge (4, 11), the last loop edge
    d = _graph(eng, g)
    rec = _prepare(eng, d)
    assert rec[1] == 1 and rec[13] == 0 and rec[14] == 1
    less = _graph(eng, _cut(g, d["loops"] - 1))                      # the graph without that edge
    _prepare(eng, less)
    lin = _lin(_cut(g, d["loops"] - 1))
    p = MR.prepare(g["init"], lin, g["Omega"][:-1])
    for f in MR.FRAMES:
        got = _marg(eng, d, np.arange(16), f)
        assert np.isfinite(got).all() and d["buf"]["record"].cpu().numpy()[7] == 0
        assert MR.distance(got, _marg(eng, less, np.arange(16), f), p) <= 1e-12
        assert MR.distance(got, MR.dense_marginals(lin, g["init"], f), p) <= 1e-9


def test_zero_information_on_a_loop_edge_breaks_down_and_leaves_cov_untouched(eng, ref):
    g = dict(ref["n16_loop1"]["g"])
    g["Omega"] = g["Omega"].copy()
    g["Omega"][-1] = 0.0
    d = _graph(eng, g)
    rec = _prepare(eng, d)
    assert rec[2] == 0 and rec[13] == 1 and rec[14] == 0
    cov = torch.full((16, 6, 6), 7.0, dtype=torch.float64, device=eng.device)
    _marg(eng, d, np.arange(16), "position", cov=cov)
    r = d["buf"]["record"].cpu().numpy()
    assert r[7] == 1 and r[15] == 0 and np.all(cov.cpu().numpy() == 7.0)
    from overlapnet_amd._lib import OvnError
    from overlapnet_amd.pose_graph import PoseGraph
    pg = PoseGraph(eng, g["init"])
    pg._ij, pg._z, pg._info = [tuple(e) for e in g["edges"]], list(g["Z"]), list(g["Omega"])     # past add_edge's refusal
    with pytest.raises(OvnError, match="not positive"):
        pg.marginals()
    g["Omega"][-1] = ref["n16_loop1"]["g"]["Omega"][-1]                # a good prepare on the same record clears `breakdown`
    d2 = _graph(eng, g)
    d2["buf"]["record"] = d["buf"]["record"]
    _prepare(eng, d2)
    got = _marg(eng, d2, np.arange(16), "position")
    assert d["buf"]["record"].cpu().numpy()[7] == 0 and np.array_equal(got, _marg(eng, d2, np.arange(16), "position"))


def test_an_id_outside_the_graph_gives_nans_and_is_counted(eng, ref):
    c = ref["n64_loop2"]
    d = _graph(eng, c["g"])
    _prepare(eng, d)
    ids = np.array([3, -1, 5, 64, 7, 2 ** 31 - 1, 63, -2 ** 31, 9, 10, 11], np.int64)
    for f in MR.FRAMES:
        every = _marg(eng, d, np.arange(64), f)
        got = _marg(eng, d, ids, f)
        r = d["buf"]["record"].cpu().numpy()
        assert r[15] == 4 and r[7] == 0
        for k, S in zip(ids, got):
            assert np.isnan(S).all() if not 0 <= k < 64 else np.array_equal(_bits(S), _bits(every[k]))
        _marg(eng, d, [5], f)
        assert d["buf"]["record"].cpu().numpy()[15] == 0


def test_argument_errors(eng, ref):
    c = ref["n16_outlier"]
    d = _graph(eng, c["g"])
    _prepare(eng, d)
    lib, h, s = eng.lib, eng._h, eng._stream()
    p = lambda t: None if t is None else t.data_ptr()
    b = d["buf"]
    n, e, L = d["n"], d["e"], d["loops"]
    ids = _up(eng, np.arange(n, dtype=np.int32))
    cov = torch.full((n, 6, 6), 7.0, dtype=torch.float64, device=eng.device)
    ws = torch.full((eng.pose_graph_marginals_bytes(n, L, n) // 8,), 7.0, dtype=torch.float64, device=eng.device)
    before = {k: v.clone() for k, v in b.items()}

    def call(**kw):
        a = dict(poses=p(d["poses"]), n=n, e=e, L=L, chain=p(b["chain"]), loops=p(b["loops"]), ids=p(ids), k=n, frame=1, cov=p(cov),
                 ws=p(ws), rec=p(b["record"]))
        a.update(kw)
        return lib.ovn_pose_graph_marginals(h, s, a["poses"], a["n"], a["e"], a["L"], a["chain"], a["loops"], a["ids"], a["k"],
                                            a["frame"], a["cov"], a["ws"], a["rec"])

    for kw in [dict(n=1, e=L), dict(n=(1 << 20) + 1), dict(L=-1), dict(L=LR.MAX_LOOPS + 1, e=n + LR.MAX_LOOPS), dict(e=e + 1),
               dict(e=e - 1), dict(L=L + 1), dict(L=L - 1), dict(L=0), dict(k=0), dict(k=-1), dict(k=(1 << 22) + 1), dict(frame=2),
               dict(frame=-1), dict(poses=None), dict(chain=None), dict(loops=None), dict(ids=None), dict(cov=None), dict(ws=None),
               dict(rec=None)]:
        assert call(**kw) == 1, kw
        assert lib.ovn_last_error()
    assert lib.ovn_pose_graph_marginals(None, s, p(d["poses"]), n, e, L, p(b["chain"]), p(b["loops"]), p(ids), n, 1, p(cov), p(ws),
                                        p(b["record"])) == 1
    torch.cuda.synchronize()
    for k, v in b.items():
        assert torch.equal(v.view(torch.int64), before[k].view(torch.int64)), "a refused call wrote %s" % k
    assert np.all(cov.cpu().numpy() == 7.0) and np.all(ws.cpu().numpy() == 7.0)
    assert call() == 0 and call(L=0, e=n - 1, loops=None) == 0      # L = 0 does not read loops_dev
    torch.cuda.synchronize()
    assert np.isfinite(cov.cpu().numpy()).all()
    from overlapnet_amd._lib import OvnError
    with pytest.raises(OvnError, match="no frame"):
        _marg(eng, d, [1], "world")
    with pytest.raises(OvnError, match="ws holds"):
        _marg(eng, d, np.arange(n), "local", ws=ws[:4])
    with pytest.raises(OvnError, match="node_ids"):
        eng.pose_graph_marginals(d["poses"], b, ids.to(torch.int64), L)


def test_pose_graph_marginals_after_optimize_is_the_direct_call(eng, ref):
    from overlapnet_amd.pose_graph import PoseGraph
    g = ref["n64_loop2"]["g"]
    pg = PoseGraph(eng, g["init"], fixed=np.flatnonzero(g["fixed"]))
    for (i, j), Z, om in zip(g["edges"], g["Z"], g["Omega"]):
        pg.add_edge(i, j, Z, om)
    res = pg.optimize(preconditioner="loops")
    assert res.converged and np.array_equal(pg.poses, res.poses)
    at = dict(g)
    at["init"] = res.poses
    d = _graph(eng, at)
    _prepare(eng, d)
    for f in MR.FRAMES:
        direct = _marg(eng, d, np.arange(64), f)
        assert np.array_equal(_bits(pg.marginals(frame=f)), _bits(direct))
        assert np.array_equal(_bits(pg.marginals(nodes=[63, 1, 1], frame=f)), _bits(direct[[63, 1, 1]]))
    assert np.array_equal(_bits(pg.marginals()), _bits(_marg(eng, d, np.arange(64), "position")))
    assert np.array_equal(_bits(pg.marginals(poses=g["init"], frame="local")),
                          _bits(_marg(eng, _prepared(eng, g), np.arange(64), "local")))
    lin = R.linearize(res.poses, g["fixed"], g["edges"], g["Z"], g["Omega"], g["huber"])
    p = MR.prepare(res.poses, lin, g["Omega"])
    assert MR.distance(pg.marginals(), MR.dense_marginals(lin, res.poses, "position"), p) <= 1e-9
    chain = PoseGraph(eng, g["init"])                                # L = 0: dead reckoning
    chain.add_odometry(g["Z"][:63], g["Omega"][0])
    lin0 = _lin(_cut(g, 0))
    want = MR.marginals(MR.prepare(g["init"], lin0, g["Omega"][:63]), g["init"], range(64), "position")
    assert MR.distance(chain.marginals(), want, p) <= 1e-12


def test_the_covariance_file_and_the_gate_from_gpu_marginals(eng, tmp_path):
    """What tools/slam.py does with --gate-sigma and --covariances, without the network: the odometry-only graph's marginals in the
    position frame, written, read back, turned into ellipses, and the candidate lists of tests/golden/pose_graph_marginals.json."""
    import json
    import os
    from overlapnet_amd import lcd
    from overlapnet_amd.pose_graph import PoseGraph
    g, d = MR.GATE, MR.gate_drive()
    pg = PoseGraph(eng, d["init"])
    pg.add_odometry(d["Z"], d["Omega"][0])
    cov = pg.marginals(frame="position")
    path = str(tmp_path / "covariance.txt")
    lcd.write_covariances(path, cov)
    back = lcd.read_covariances(path)
    assert back.shape == (g["frames"], 6, 6) and np.array_equal(_bits(back), _bits(cov))
    lin = _lin(d)
    p = MR.prepare(d["init"], lin, d["Omega"])
    fwd, rev = MR.marginals(p, d["init"], range(g["frames"]), "position"), \
        MR.marginals(MR.prepare(d["init"], lin, d["Omega"], True), d["init"], range(g["frames"]), "position", True)
    assert MR.distance(cov, fwd, p) <= 10 * MR.distance(rev, fwd, p)
    ell = lcd.ellipses_from_covariances(back, g["nstd"])
    xy = d["init"][:, :2, 3]
    length = lcd.travelled_distances(xy)
    got = {str(k): [int(v) for v in lcd.gate_candidates(k, xy, length, ell[k], inactive_time_thres=g["min_gap"] - 1,
                                                        inactive_dist_thres=-np.inf)] for k in range(g["frames"])}
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_marginals.json")))
    assert {k: v for k, v in got.items() if v} == gold["candidates"]


def _prepared(eng, g):
    d = _graph(eng, g)
    _prepare(eng, d)
    return d
