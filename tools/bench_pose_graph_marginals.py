"""Timing of the marginal covariances (ovn_pose_graph_marginals, csrc/pose_graph.hip) on the drives of
tools/bench_pose_graph.py: two laps of a circle, N = 1024, 4096, 16384 poses and L = 0, 1, 32, 128, 256 loop edges.  Per graph, in one
run, after one linearization and (for L >= 1) one ovn_pose_graph_loops_prepare:

  all_nodes_ms      the call for all N nodes in the position frame (HIP events around windows of at least --min-ms of device time,
                    median of --rounds), and the sweep's nominal fp64 rate 6 N sp^2 / time (one multiply and one add per entry of the
                    lower triangle of the factor and column; sp is the padded order of S; leading block rows that are skipped for a tile
                    are counted as if they were walked, so the figure is a lower bound of the rate on the work done)
  one_node_ms       the call for the last node alone: the online case
  cpu               the same blocks on the CPU: scipy.sparse.linalg.splu of the same reduced Hessian, then its solve with the 6 unit
                    columns of each queried node, of which the diagonal block is kept.  One node: measured.  All nodes: the factorization
                    and the columns of --cpu-nodes nodes spread over the drive are measured, and the figure for all N is the factorization
                    plus N / --cpu-nodes times the columns' time -- an extrapolation, and said to be one (6 N solves of order 6 N at N =
                    16384 are minutes).  Without scipy: numpy.linalg.inv up to the N where that takes under a minute, and which was used
                    is recorded.
  agreement         the largest distance of the GPU's blocks from the CPU's over the measured nodes, relative to the largest GPU entry

No figure is promised; ONE JSON object on stdout.

    python tools/bench_pose_graph_marginals.py > profiles/pose_graph_marginals.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pose_graph import drive  # noqa: E402
from tools.bench_raycast import alternating  # noqa: E402

DENSE_MAX_NODES = 2048      # numpy.linalg.inv of order 6 N: under a minute up to here


def hessian(n, edges, blocks):
    """The reduced Hessian (node 0 removed) as a dense-block COO triple: rows, columns, values."""
    i, j = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    rows = np.concatenate([i, i, j, j])
    cols = np.concatenate([i, j, i, j])
    data = np.concatenate([blocks[:, 0], blocks[:, 1], np.swapaxes(blocks[:, 1], 1, 2), blocks[:, 2]])
    r6 = (6 * rows[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64)).ravel()
    c6 = (6 * cols[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)).ravel()
    return r6, c6, data.ravel()


def cpu_blocks(n, edges, blocks, nodes):
    """-> (what was used, seconds to factor, seconds for the nodes' columns, (len(nodes),6,6) local-frame blocks)."""
    r6, c6, data = hessian(n, edges, blocks)
    nodes = [int(k) for k in nodes]
    try:
        import scipy
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu
    except Exception:  # noqa: BLE001
        if n > DENSE_MAX_NODES:
            return "numpy.linalg.inv: not run above %d nodes" % DENSE_MAX_NODES, None, None, None
        H = np.zeros((6 * n, 6 * n))
        np.add.at(H, (r6, c6), data)
        t0 = time.perf_counter()
        Hi = np.linalg.inv(H[6:, 6:])
        t1 = time.perf_counter()
        return "numpy.linalg.inv", t1 - t0, 0.0, np.stack([Hi[6 * k - 6:6 * k, 6 * k - 6:6 * k] for k in nodes])
    H = sp.coo_matrix((data, (r6, c6)), shape=(6 * n, 6 * n)).tocsc()[6:, 6:]
    t0 = time.perf_counter()
    lu = splu(H)
    t1 = time.perf_counter()
    out = np.zeros((len(nodes), 6, 6))
    for c, k in enumerate(nodes):
        rhs = np.zeros((6 * (n - 1), 6))
        rhs[6 * (k - 1) + np.arange(6), np.arange(6)] = 1.0
        out[c] = lu.solve(rhs)[6 * (k - 1):6 * k]
    t2 = time.perf_counter()
    return "scipy.sparse.linalg.splu " + scipy.__version__, t1 - t0, t2 - t1, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--loops", type=int, nargs="+", default=[0, 1, 32, 128, 256])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cpu-nodes", type=int, default=64, help="nodes whose columns the CPU solves for the all-nodes figure")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph_marginals needs the MI355X: there is no CPU path and no figure to report without it")
    from overlapnet_amd.engine import OvnEngine
    from overlapnet_amd import pose_graph as PG
    torch.cuda.set_device(0)
    eng = OvnEngine(64, 900, 1, device=0)
    om = PG.information_from_sigmas(0.05, 0.01)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    out = {"device": torch.cuda.get_device_name(0), "args": vars(args), "cases": []}
    for n in args.nodes:
        for L in args.loops:
            _, start, edges, Z = drive(n, L)
            e = len(edges)
            fixed_h = np.zeros(n, np.uint8)
            fixed_h[0] = 1
            ptr, lst = (up(a) for a in PG.incidence(n, edges))
            poses, fixed, ij, meas, info = up(start), up(fixed_h), up(edges), up(Z), up(np.tile(om, (e, 1, 1)))
            buf = eng.pose_graph_buffers(n, e, chain=True, loops=L)
            eng.pose_graph_linearize(poses, fixed, ij, meas, info, ptr, lst, float("inf"), buf)
            if L:
                eng.pose_graph_loops_prepare(poses, ij, info, buf)
            sp = (6 * L + 47) // 48 * 48
            every, last = up(np.arange(n, dtype=np.int32)), up(np.array([n - 1], np.int32))
            nbytes = eng.pose_graph_marginals_bytes(n, L, n)
            ws = torch.empty(nbytes // 8, dtype=torch.float64, device=eng.device)
            cov_all = torch.zeros((n, 6, 6), dtype=torch.float64, device=eng.device)
            cov_one = torch.zeros((1, 6, 6), dtype=torch.float64, device=eng.device)
            fns = {"all": lambda: eng.pose_graph_marginals(poses, buf, every, L, "position", cov=cov_all, ws=ws),
                   "one": lambda: eng.pose_graph_marginals(poses, buf, last, L, "position", cov=cov_one, ws=ws)}
            t = alternating(fns, args.warmup, args.min_ms, args.rounds)
            rec = buf["record"].cpu().numpy()
            flops = 6.0 * n * sp * sp
            case = {"nodes": n, "loops": L, "order_of_S": sp, "workspace_bytes": nbytes, "record_7_13_15": [float(rec[7]), float(rec[13]), float(rec[15])],
                    "all_nodes_ms": round(t["all"][0], 5), "all_nodes_windows": t["all"][1], "one_node_ms": round(t["one"][0], 5),
                    "one_node_windows": t["one"][1], "sweep_nominal_flop": flops,
                    "sweep_nominal_tflops": round(flops / (t["all"][0] * 1e-3) / 1e12, 4) if L else None}
            # the CPU: the local-frame blocks of the sampled nodes, against the GPU's
            sample = sorted(set(np.linspace(1, n - 1, args.cpu_nodes).astype(int).tolist()))
            used, t_factor, t_cols, blocks = cpu_blocks(n, edges, buf["blocks"].cpu().numpy(), sample)
            cpu = {"used": used}
            if blocks is not None:
                local = eng.pose_graph_marginals(poses, buf, up(np.asarray(sample, np.int32)), L, "local").cpu().numpy()
                cpu.update(factor_ms=round(1e3 * t_factor, 3), sampled_nodes=len(sample), sampled_columns_ms=round(1e3 * t_cols, 3),
                           all_nodes_ms_extrapolated=round(1e3 * (t_factor + t_cols * n / len(sample)), 1),
                           agreement=float(np.abs(local - blocks).max() / np.abs(local).max()))
                _, f1, c1, _ = cpu_blocks(n, edges, buf["blocks"].cpu().numpy(), [n - 1])
                cpu["one_node_ms"] = round(1e3 * (f1 + c1), 3)
            case["cpu"] = cpu
            out["cases"].append(case)
            print("done N = %d, L = %d: all %.3f ms, one %.3f ms, cpu %s" % (n, L, t["all"][0], t["one"][0], json.dumps(cpu)),
                  file=sys.stderr, flush=True)
            del buf, ws
            torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
