"""Timing of the pose-graph optimizer (csrc/pose_graph.hip, overlapnet_amd/pose_graph.py).

Graphs: a synthetic drive of N poses, two laps of a circle with 0.5 m steps (so the second lap revisits the first), odometry noise
0.02 m / 0.004 rad, Omega = diag(1 / 0.05^2 x 3, 1 / 0.01^2 x 3), node 0 fixed, L loop edges (k + N / 2, k) spread evenly over the
first lap; the start is dead reckoning.  N = 1024, 4096, 16384 and L = 1, 32, 512.  Per graph and preconditioner (jacobi, chain):

  linearize_ms      one full linearization (HIP events around windows of at least --min-ms of device time, median of --rounds)
  pcg_iteration_ms  one PCG iteration: a solve of 64 iterations from its start, rtol 0, the same way, divided by 64
  pcg_iterations    iterations of the first solve to rtol 1e-8 (capped at --max-cg), and its wall time
  optimize          a whole `PoseGraph.optimize` (at most --outer outer iterations, --max-cg per solve): wall seconds, iterations, costs
  cpu_spsolve_s     one outer step on the CPU: scipy.sparse.linalg.spsolve on the same matrix (the blocks copied back), or the reason
                    it is missing

No figure is promised; ONE JSON object on stdout.

    python tools/bench_pose_graph.py > profiles/pose_graph.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_raycast import alternating  # noqa: E402


def _exp(xi):
    """Exp of (n,6) twists (v, omega) -> (n,4,4), Rodrigues."""
    v, w = xi[:, :3], xi[:, 3:]
    th = np.linalg.norm(w, axis=1)
    small = th < 1e-6
    t = np.where(small, 1.0, th)
    a, b, c = np.where(small, 1.0, np.sin(t) / t), np.where(small, 0.5, (1 - np.cos(t)) / t ** 2), np.where(small, 1 / 6, (t - np.sin(t)) / t ** 3)
    W = np.zeros((len(xi), 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    W2 = W @ W
    T = np.tile(np.eye(4), (len(xi), 1, 1))
    T[:, :3, :3] += a[:, None, None] * W + b[:, None, None] * W2
    T[:, :3, 3] = np.einsum("nab,nb->na", np.eye(3) + b[:, None, None] * W + c[:, None, None] * W2, v)
    return T


def drive(n, loops, seed=0):
    """-> (true (n,4,4), start (n,4,4), edges (E,2), Z (E,4,4))."""
    rng = np.random.default_rng([seed, n, loops])
    ang = 4.0 * np.pi * np.arange(n) / n
    radius = 0.5 * n / (4.0 * np.pi)
    true = _exp(np.concatenate([np.zeros((n, 5)), (ang + 0.5 * np.pi)[:, None]], 1))
    true[:, :3, 3] = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.2 * np.sin(3 * ang)], 1)
    half = n // 2
    ks = (np.arange(loops) * half) // loops
    edges = np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], 1), np.stack([ks + half, ks], 1)]).astype(np.int32)
    inv = np.linalg.inv(true)
    noise = _exp(rng.standard_normal((len(edges), 6)) * np.array([0.02] * 3 + [0.004] * 3))
    Z = inv[edges[:, 0]] @ true[edges[:, 1]] @ noise
    start = [true[0]]
    for k in range(n - 1):
        start.append(start[-1] @ Z[k])
    return true, np.stack(start), edges, Z


def cpu_spsolve(n, edges, blocks, grad):
    """Seconds of scipy's sparse direct solve of H delta = -g over the free nodes 1 .. n - 1, and |delta|_inf."""
    try:
        import scipy
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve
    except Exception as e:  # noqa: BLE001
        return {"missing": "scipy: %s" % e}
    i, j = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    rows = np.concatenate([i, i, j, j])
    cols = np.concatenate([i, j, i, j])
    data = np.concatenate([blocks[:, 0], blocks[:, 1], np.swapaxes(blocks[:, 1], 1, 2), blocks[:, 2]])
    r6 = (6 * rows[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64)).ravel()
    c6 = (6 * cols[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)).ravel()
    H = sp.coo_matrix((data.ravel(), (r6, c6)), shape=(6 * n, 6 * n)).tocsc()[6:, 6:]
    b = -grad[1:].ravel()
    t0 = time.perf_counter()
    x = spsolve(H, b)
    dt = time.perf_counter() - t0
    return {"seconds": round(dt, 5), "delta_max": float(np.abs(x).max()), "scipy": scipy.__version__, "nnz": int(H.nnz)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--loops", type=int, nargs="+", default=[1, 32, 512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--outer", type=int, default=6)
    ap.add_argument("--max-cg", type=int, default=40000)
    args = ap.parse_args(argv)
    from overlapnet_amd.engine import OvnEngine
    from overlapnet_amd import pose_graph as PG
    torch.cuda.set_device(0)
    eng = OvnEngine(64, 900, 1, device=0)
    om = PG.information_from_sigmas(0.05, 0.01)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    out = {"device": torch.cuda.get_device_name(0), "args": vars(args), "cases": []}
    for n in args.nodes:
        for L in args.loops:
            true, start, edges, Z = drive(n, L)
            e = len(edges)
            fixed_h = np.zeros(n, np.uint8)
            fixed_h[0] = 1
            ptr, lst = (up(a) for a in PG.incidence(n, edges))
            poses, fixed, ij, meas, info = up(start), up(fixed_h), up(edges), up(Z), up(np.tile(om, (e, 1, 1)))
            buf = eng.pose_graph_buffers(n, e, chain=True)
            lin = lambda: eng.pose_graph_linearize(poses, fixed, ij, meas, info, ptr, lst, float("inf"), buf)
            case = {"nodes": n, "loops": L, "edges": e}
            rec = lin().cpu().numpy()
            case["cost_start"] = float(rec[0])
            case["cpu_spsolve"] = cpu_spsolve(n, edges, buf["blocks"].cpu().numpy(), buf["grad"].cpu().numpy())
            fns = {"linearize": lin}
            for kind in ("jacobi", "chain"):
                fns["pcg64_" + kind] = (lambda kind=kind: eng.pose_graph_solve(fixed, ij, ptr, lst, buf, kind, 0.0, 0.0, 0, 64))
            t = alternating(fns, args.warmup, args.min_ms, args.rounds)
            case["linearize_ms"] = {"median": round(t["linearize"][0], 5), "windows": t["linearize"][1]}
            for kind in ("jacobi", "chain"):
                k = {"pcg_iteration_ms": {"median": round(t["pcg64_" + kind][0] / 64, 6), "windows_of_64": t["pcg64_" + kind][1]}}
                torch.cuda.synchronize()
                t0, done = time.perf_counter(), 0
                while True:
                    r = eng.pose_graph_solve(fixed, ij, ptr, lst, buf, kind, 0.0, 1e-8, done, 64).cpu().numpy()
                    done += 64
                    if r[6] or r[7] or done >= args.max_cg:
                        break
                k["pcg_iterations"] = {"iterations": int(r[4]), "converged": bool(r[6]), "breakdown": bool(r[7]), "relative_residual": float(r[5]),
                                       "wall_s": round(time.perf_counter() - t0, 4)}
                g = _graph(PG, eng, start, edges, Z, om)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = g.optimize(max_iterations=args.outer, preconditioner=kind, cg_chunk=64, max_cg=args.max_cg)
                torch.cuda.synchronize()
                k["optimize"] = {"wall_s": round(time.perf_counter() - t0, 4), "outer_iterations": res.outer_iterations,
                                 "cg_iterations": res.cg_iterations, "converged": bool(res.converged), "cost_initial": res.cost_initial,
                                 "cost_final": res.cost_final,
                                 "max_position_error_m": float(np.linalg.norm(res.poses[:, :3, 3] - true[:, :3, 3], axis=1).max())}
                case[kind] = k
            case["start_max_position_error_m"] = float(np.linalg.norm(start[:, :3, 3] - true[:, :3, 3], axis=1).max())
            case["auto"] = _graph(PG, eng, start, edges, Z, om).choose_preconditioner("auto")
            out["cases"].append(case)
            print("done N = %d, L = %d" % (n, L), file=sys.stderr, flush=True)
    eng.close()
    print(json.dumps(out, indent=1))


def _graph(PG, eng, start, edges, Z, om):
    n = len(start)
    g = PG.PoseGraph(eng, start)
    g.add_odometry(Z[:n - 1], om)
    for (i, j), z in zip(edges[n - 1:], Z[n - 1:]):
        g.add_edge(i, j, z, om)
    return g


if __name__ == "__main__":
    main()
