"""SE(3) pose-graph optimization on the GPU: the back end that turns verified loop closures into corrected poses.

`odometry` tracks scans into poses, `Infer.infer_top_k` proposes loop closures and `Infer.verify_top_k` checks them by ICP; this module
distributes the loop error over the trajectory.  Nodes are poses (4,4) sensor to world; an edge (i, j, Z, Omega) measures
T_i^-1 T_j with information Omega (6 x 6, twist order (v, omega)).  The statement -- residual, Jacobians, Huber weights, normal
equations, preconditioners -- is in include/ovn_hip.h and DESIGN.md section 32; the kernels are csrc/pose_graph.hip.  A drive with
many loop closures has a third preconditioner, "loops" (DESIGN.md section 33): the exact inverse of the undamped Hessian of the
odometry chain plus up to MAX_LOOPS loop edges, prepared after every full linearization.  `PoseGraph.marginals` returns that
inverse's diagonal blocks, the marginal pose covariances: the covariance file and search ellipses of `lcd`.

The outer loop is Levenberg-Marquardt on the host and reads one 16-double record per step (plus one per chunk of conjugate-gradient
iterations): lambda starts at 0 (Gauss-Newton); a trial step T Exp(delta) is accepted when the cost does not rise, then lambda <-
lambda / 10, and 0 once that is at most LAMBDA_FIRST; a rejected step sets lambda <- LAMBDA_FIRST from 0, else 10 lambda, and the loop
gives up above LAMBDA_MAX.  It stops, converged, after a solve whose |delta|_inf is at most XTOL."""
from __future__ import annotations

import collections
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

LAMBDA_FIRST = 1e-6
LAMBDA_MAX = 1e8
XTOL = 1e-10
# "auto": with the chain preconditioner conjugate gradients need about 6 L + 1 iterations for L loop edges (M^-1 H is the identity plus
# a term of rank 6 L); with block-Jacobi they needed 2.9 N .. 7.8 N on the drives of tools/bench_pose_graph.py (N = 1024 .. 16384,
# L = 1 .. 512; profiles/pose_graph.json).  The smallest measured figure is the estimate.
JACOBI_ITERATIONS_PER_NODE = 2.9
# "loops" / "auto+loops": the chain-plus-loops inverse takes at most MAX_LOOPS loop edges
# (OVN_POSE_GRAPH_MAX_LOOPS).  On the drives of tools/bench_pose_graph_loops.py (N = 1024 .. 16384; profiles/pose_graph_loops.json) one
# undamped outer step -- prepare plus solve -- took 0.7 / 0.9 .. 1.2 / 2.5 .. 3.1 / 5.5 .. 6.7 ms at L = 1 / 32 / 128 / 256, against
# 1.9 .. 2.0 / 9 .. 177 / 23 .. 698 / 34 .. 1345 ms with the chain and 2.8 .. 49 / 5.4 .. 121 / 5.2 .. 111 / 5.5 .. 103 ms for the CPU's
# sparse direct solve, and a whole optimize was faster than the chain's in all twelve cells; at L = 512 it took 13.3 ms against the
# CPU's 6.0 ms at N = 1024, which is what set MAX_LOOPS.  So "auto+loops" takes it for every L in LOOPS_MIN .. MAX_LOOPS when the
# chain precondition holds, and is "auto" otherwise.
MAX_LOOPS = 256
LOOPS_MIN = 1

Result = collections.namedtuple("Result", "poses cost_initial cost_final outer_iterations cg_iterations converged chi2 weights")


def information_from_sigmas(sigma_t: float, sigma_r: float) -> np.ndarray:
    """The diagonal information matrix of a measurement with standard deviations sigma_t [m] and sigma_r [rad]."""
    st, sr = float(sigma_t), float(sigma_r)
    if not (np.isfinite(st) and np.isfinite(sr) and st > 0.0 and sr > 0.0):
        raise ValueError("information_from_sigmas: sigmas must be finite and > 0, got %r, %r" % (sigma_t, sigma_r))
    return np.diag([1.0 / st ** 2] * 3 + [1.0 / sr ** 2] * 3)


def _relative(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a^-1 b of two (4,4) poses."""
    out = np.eye(4)
    out[:3, :3] = a[:3, :3].T @ b[:3, :3]
    out[:3, 3] = a[:3, :3].T @ (b[:3, 3] - a[:3, 3])
    return out


def incidence(n: int, edges: np.ndarray):
    """CSR incidence list of the graph: node_ptr (n + 1) and node_edge (2 E) int32, a node's edges in ascending edge index."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    e = edges.shape[0]
    node = edges.reshape(-1)                                  # entry 2 e + side
    order = np.argsort(node, kind="stable")                   # stable: ascending edge index inside a node
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, node + 1, 1)
    return np.cumsum(ptr).astype(np.int32), (order // 2).astype(np.int32).reshape(2 * e)


class PoseGraph:
    """A pose graph on one engine's GPU.  poses: (N,4,4) sensor to world, the start of the optimization; fixed: the nodes that do not
    move."""

    def __init__(self, engine, poses, fixed: Sequence[int] = (0,)):
        p = np.array(poses, np.float64)
        if p.ndim != 3 or p.shape[1:] != (4, 4) or p.shape[0] < 1:
            raise ValueError("poses must be (N,4,4) with N >= 1, got %s" % (p.shape,))
        self.engine = engine
        self.poses = p
        self.n = p.shape[0]
        f = np.zeros(self.n, bool)
        for v in fixed:
            if not 0 <= int(v) < self.n:
                raise ValueError("fixed node %d outside 0..%d" % (int(v), self.n - 1))
            f[int(v)] = True
        self.fixed = f
        self._ij, self._z, self._info = [], [], []
        self.fallbacks = 0      # outer iterations of "loops" whose factorization broke down and which the chain solved instead

    # -- building ---------------------------------------------------------------------------------------------------------------------
    def add_edge(self, i: int, j: int, Z, information) -> int:
        """Edge (i, j): Z (4,4) measures T_i^-1 T_j with information matrix `information` (6,6) SPD.  Returns the edge's index."""
        i, j = int(i), int(j)
        if not (0 <= i < self.n and 0 <= j < self.n):
            raise ValueError("edge (%d, %d): index outside 0..%d" % (i, j, self.n - 1))
        if i == j:
            raise ValueError("edge (%d, %d) joins a node to itself" % (i, j))
        Z = np.asarray(Z, np.float64)
        om = np.asarray(information, np.float64)
        if Z.shape != (4, 4) or om.shape != (6, 6):
            raise ValueError("edge (%d, %d): Z must be (4,4) and information (6,6), got %s and %s" % (i, j, Z.shape, om.shape))
        if not np.isfinite(om).all() or not np.allclose(om, om.T, rtol=1e-12, atol=0.0) or np.linalg.eigvalsh(0.5 * (om + om.T)).min() <= 0.0:
            raise ValueError("edge (%d, %d): information must be symmetric positive definite" % (i, j))
        self._ij.append((i, j))
        self._z.append(Z.copy())
        self._info.append(om.copy())
        return len(self._ij) - 1

    def add_odometry(self, poses_or_steps, information) -> None:
        """The N - 1 odometry edges (k, k + 1).  poses_or_steps: (N,4,4) poses, whose steps T_k^-1 T_{k+1} are taken, or (N-1,4,4) steps."""
        a = np.asarray(poses_or_steps, np.float64)
        if a.ndim != 3 or a.shape[1:] != (4, 4) or a.shape[0] not in (self.n, self.n - 1):
            raise ValueError("add_odometry: (%d,4,4) poses or (%d,4,4) steps, got %s" % (self.n, self.n - 1, a.shape))
        steps = a if a.shape[0] == self.n - 1 else [_relative(a[k], a[k + 1]) for k in range(self.n - 1)]
        for k in range(self.n - 1):
            self.add_edge(k, k + 1, steps[k], information)

    def add_loop_closures(self, current_id: int, verified, information, only_accepted: bool = True) -> int:
        """The list `Infer.verify_top_k(current_id, ...)` returns -- (reference id, overlap, yaw, pose, fitness, rms, accepted) -- as
        edges (current_id, reference id, pose): the pose takes the reference scan's points into the current scan's frame, which is
        T_current^-1 T_reference.  only_accepted=True keeps the candidates whose `accepted` is True (None, no threshold given to
        verify_top_k, is refused: this library chooses none).  Returns the number of edges added."""
        added = 0
        for rec in verified:
            ref, pose, accepted = int(rec[0]), rec[3], rec[6]
            if only_accepted:
                if accepted is None:
                    raise ValueError("add_loop_closures: verify_top_k ran without min_fitness / max_rms, so nothing says which candidates "
                                     "to accept; give it a threshold or pass only_accepted=False")
                if not accepted:
                    continue
            if not np.isfinite(np.asarray(pose, np.float64)).all():
                continue
            self.add_edge(int(current_id), ref, pose, information)
            added += 1
        return added

    @property
    def edges(self) -> np.ndarray:
        return np.asarray(self._ij, np.int32).reshape(-1, 2)

    # -- checks before the GPU -------------------------------------------------------------------------------------------------------------
    def chain_available(self) -> bool:
        """Edges 0 .. N - 2 are exactly (k, k + 1) in order and node 0 is the only fixed node."""
        e = self.edges
        return (self.n >= 2 and e.shape[0] >= self.n - 1 and bool(self.fixed[0]) and int(self.fixed.sum()) == 1
                and np.array_equal(e[:self.n - 1], np.stack([np.arange(self.n - 1), np.arange(1, self.n)], 1)))

    def _check(self) -> None:
        if not self.fixed.any():
            raise ValueError("the graph has no fixed node: its gauge is free")
        e = self.edges.astype(np.int64)
        deg = np.bincount(e.reshape(-1), minlength=self.n)
        lonely = np.flatnonzero((deg == 0) & ~self.fixed)
        if lonely.size:
            raise ValueError("free node %d has no edge" % int(lonely[0]))
        parent = np.arange(self.n)

        def find(v):
            while parent[v] != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v
        for i, j in e:
            a, b = find(int(i)), find(int(j))
            if a != b:
                parent[b] = a
        roots = np.array([find(v) for v in range(self.n)])
        anchored = set(roots[self.fixed].tolist())
        for v in range(self.n):
            if roots[v] not in anchored:
                raise ValueError("node %d lies in a component without a fixed node" % v)

    @property
    def loops(self) -> int:
        """The number of edges after the N - 1 a chain would take."""
        return len(self._ij) - (self.n - 1)

    def choose_preconditioner(self, preconditioner: str = "auto") -> str:
        if preconditioner == "jacobi":
            return "jacobi"
        if preconditioner == "loops":
            if not self.chain_available():
                raise ValueError("the chain-plus-loops inverse needs edges 0 .. N - 2 to be the odometry steps (k, k + 1) in order and "
                                 "node 0 to be the only fixed node")
            if not 1 <= self.loops <= MAX_LOOPS:
                raise ValueError("the chain-plus-loops inverse takes 1 .. %d loop edges after the chain, the graph has %d"
                                 % (MAX_LOOPS, self.loops))
            return "loops"
        if preconditioner == "auto+loops":
            if self.chain_available() and LOOPS_MIN <= self.loops <= MAX_LOOPS:
                return "loops"
            preconditioner = "auto"
        if preconditioner == "chain":
            if not self.chain_available():
                raise ValueError("the chain preconditioner needs edges 0 .. N - 2 to be the odometry steps (k, k + 1) in order and node 0 "
                                 "to be the only fixed node")
            return "chain"
        if preconditioner != "auto":
            raise ValueError("no preconditioner %r (auto, auto+loops, jacobi, chain, loops)" % (preconditioner,))
        loops = len(self._ij) - (self.n - 1)
        if self.chain_available() and 6 * loops + 1 < JACOBI_ITERATIONS_PER_NODE * self.n:
            return "chain"
        return "jacobi"

    # -- optimization ----------------------------------------------------------------------------------------------------------------------
    def optimize(self, max_iterations: int = 30, huber: Optional[float] = None, preconditioner: str = "auto", rtol: float = 1e-8,
                 cg_chunk: int = 32, max_cg: int = 100000) -> Result:
        """Levenberg-Marquardt with preconditioned conjugate gradients on the GPU (schedule: module docstring).  huber: threshold of the
        robust kernel on s = sqrt(r' Omega r), None = least squares.  rtol: the relative M-norm residual at which a solve stops; it is
        enqueued in chunks of cg_chunk iterations between which the host reads the solver's record, at most max_cg per solve.
        Returns Result(poses (N,4,4), cost_initial, cost_final, outer_iterations, cg_iterations, converged, chi2 (E), weights (E));
        chi2 = r' Omega r and the weights at the result show which edges the robust kernel turned down.  self.poses is updated."""
        self._check()
        k = float("inf") if huber is None else float(huber)
        if not k > 0.0:
            raise ValueError("huber must be > 0 (None: least squares), got %r" % (huber,))
        if not (rtol >= 0.0 and np.isfinite(rtol)):
            raise ValueError("rtol must be finite and >= 0, got %r" % (rtol,))
        cg_chunk = int(cg_chunk)
        if cg_chunk < 1:
            raise ValueError("cg_chunk must be >= 1, got %d" % cg_chunk)
        kind = self.choose_preconditioner(preconditioner)
        eng, dev = self.engine, self.engine.device
        e = len(self._ij)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ij = up(self.edges)
        meas = up(np.asarray(self._z, np.float64).reshape(e, 4, 4))
        info = up(np.asarray(self._info, np.float64).reshape(e, 6, 6))
        fixed = up(self.fixed.astype(np.uint8))
        ptr, lst = (up(a) for a in incidence(self.n, self.edges))
        poses, trial = up(self.poses), torch.empty((self.n, 4, 4), dtype=torch.float64, device=dev)
        buf = eng.pose_graph_buffers(self.n, e, chain=(kind == "chain"), loops=(self.loops if kind == "loops" else 0))
        rec_trial = torch.zeros(16, dtype=torch.float64, device=dev)

        def lin(p, **kw):
            rec = eng.pose_graph_linearize(p, fixed, ij, meas, info, ptr, lst, k, buf, **kw)
            if kind == "loops" and kw.get("jacobians", True):          # the inverse belongs to this linearization
                rec = eng.pose_graph_loops_prepare(p, ij, info, buf)
            return rec.cpu().numpy()

        def refuse(rec):
            if rec[2] != 0:
                raise _lib.OvnError("pose graph: %d diagonal blocks are not positive definite (an information matrix, or a free node "
                                    "no finite edge holds)" % int(rec[2]))
        rec = lin(poses)
        refuse(rec)
        cost0 = cost = float(rec[0])
        lam, outer, cg, converged = 0.0, 0, 0, False
        while outer < int(max_iterations) and lam <= LAMBDA_MAX and e > 0:
            done = 0
            use = kind
            if kind == "loops" and rec[13] != 0:                       # S has no Cholesky factor at this linearization
                use = "chain"
                self.fallbacks += 1
            while True:
                r = eng.pose_graph_solve(fixed, ij, ptr, lst, buf, use, lam, rtol, done, min(cg_chunk, max_cg - done)).cpu().numpy()
                done += min(cg_chunk, max_cg - done)
                if r[6] != 0 or r[7] != 0 or done >= max_cg:
                    break
            cg += int(r[4])
            outer += 1
            if r[7] != 0 and r[4] == 0:
                raise _lib.OvnError("pose graph: the conjugate gradients broke down at their start (record %s)" % (r[:13],))
            eng.pose_graph_retract(poses, fixed, buf, out=trial, record=rec_trial)
            t = lin(trial, jacobians=False, record=rec_trial)
            small = float(t[12]) <= XTOL
            if float(t[0]) <= cost:
                poses, trial = trial, poses
                rec = lin(poses)
                refuse(rec)
                cost = float(rec[0])
                lam = 0.0 if lam / 10.0 <= LAMBDA_FIRST else lam / 10.0
            else:
                lin(poses, jacobians=False, record=rec_trial)    # the trial left ITS residuals and weights in the buffers
                lam = LAMBDA_FIRST if lam == 0.0 else 10.0 * lam
            if small:
                converged = True
                break
        self.poses = poses.cpu().numpy()
        chi = buf["chi"].cpu().numpy()
        return Result(self.poses.copy(), cost0, cost, outer, cg, converged, chi * chi, buf["weight"].cpu().numpy())

    # -- marginal covariances --------------------------------------------------------------------------------------------------------------
    def marginals(self, nodes=None, frame: str = "position", huber: Optional[float] = None, poses=None) -> np.ndarray:
        """(K,6,6): the marginal covariance of every node in `nodes` (None: all N, in order) -- the diagonal blocks of the inverse of
        the undamped Hessian at self.poses (`optimize` leaves them at its result; poses= takes another (N,4,4) point), relative to the
        fixed node 0, whose block is zero.  frame: "position" (position in the world, rotation vector in the
        world; the top-left 2 x 2 is the x, y covariance of a search ellipse, `lcd.ellipses_from_covariances`) or "local" (the
        optimizer's delta_k).  huber: the robust kernel whose weights the linearization takes, None = least squares.  The graph must
        be a chain plus at most MAX_LOOPS loop edges; with no loop edge the result is dead-reckoning covariance propagation."""
        if not self.chain_available():
            raise ValueError("marginal covariances need edges 0 .. N - 2 to be the odometry steps (k, k + 1) in order and node 0 to be "
                             "the only fixed node")
        if self.loops > MAX_LOOPS:
            raise ValueError("marginal covariances take at most %d loop edges after the chain, the graph has %d" % (MAX_LOOPS, self.loops))
        if frame not in ("position", "local"):
            raise ValueError("no frame %r (position, local)" % (frame,))
        k = float("inf") if huber is None else float(huber)
        if not k > 0.0:
            raise ValueError("huber must be > 0 (None: least squares), got %r" % (huber,))
        ids = np.arange(self.n, dtype=np.int32) if nodes is None else np.asarray(nodes).reshape(-1)
        if ids.size < 1:
            raise ValueError("marginals: no node asked for")
        if not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= self.n:
            raise ValueError("marginals: nodes must be integers in 0..%d" % (self.n - 1))
        p = self.poses if poses is None else np.array(poses, np.float64)
        if p.shape != (self.n, 4, 4):
            raise ValueError("poses must be (%d,4,4), got %s" % (self.n, p.shape))
        self._check()
        eng, dev = self.engine, self.engine.device
        e, nl = len(self._ij), self.loops
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        ij = up(self.edges)
        meas = up(np.asarray(self._z, np.float64).reshape(e, 4, 4))
        info = up(np.asarray(self._info, np.float64).reshape(e, 6, 6))
        fixed = up(self.fixed.astype(np.uint8))
        ptr, lst = (up(a) for a in incidence(self.n, self.edges))
        pd = up(p)
        buf = eng.pose_graph_buffers(self.n, e, chain=True, loops=nl)
        rec = eng.pose_graph_linearize(pd, fixed, ij, meas, info, ptr, lst, k, buf)
        if nl > 0:
            rec = eng.pose_graph_loops_prepare(pd, ij, info, buf)
        cov = eng.pose_graph_marginals(pd, buf, up(ids.astype(np.int32)), nl, frame=frame)
        r = buf["record"].cpu().numpy()
        if r[7] != 0:
            raise _lib.OvnError("marginal covariances: %d diagonal blocks and %d pivots of the loop edges' factorization are not positive "
                                "(an information matrix, or a free node no finite edge holds)" % (int(r[2]), int(r[13])))
        return cov.cpu().numpy()
