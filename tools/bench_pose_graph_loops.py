"""Timing of the chain-plus-loops inverse (ovn_pose_graph_loops_*, csrc/pose_graph.hip) on the drives of
tools/bench_pose_graph.py: two laps of a circle, N = 1024, 4096, 16384 poses and L = 1, 32, 512 loop edges -- the nine cells of
section 32's table -- and L = 128, 256 between them, which place OVN_POSE_GRAPH_MAX_LOOPS.  Per graph, in one run:

  prepare_ms        ovn_pose_graph_loops_prepare and its three stages asked for one at a time: scan (Gamma), assembly (C, the spans, S),
                    and assembly + factorization, from which `factor` is the difference (HIP events around windows of at least
                    --min-ms of device time, median of --rounds)
  apply_ms          H^-1 r alone (ovn_pose_graph_precondition_loops), beside the chain preconditioner's
  pcg_iteration_ms  (a solve of 6 iterations - a solve of 2) / 4 at lambda = 1e-6, rtol 0, for loops; chain: a solve of 64 / 64
  lam0, lam1e-6     iterations of one solve to rtol 1e-8 and its wall time with the record read back every 8 iterations, loops and chain
                    (chain capped at --max-cg)
  optimize          a whole PoseGraph.optimize (at most --outer outer iterations), loops and chain
  cpu_spsolve       scipy.sparse.linalg.spsolve on the same matrix, as tools/bench_pose_graph.py takes it

L = 512 is above OVN_POSE_GRAPH_MAX_LOOPS as shipped (the table is what lowered it): those cells are skipped, and said to be, unless
OVN_LIB names a library whose pose_graph.hip was compiled with -DOVN_POSE_GRAPH_MAX_LOOPS=512, as for profiles/pose_graph_loops.json.

No figure is promised; ONE JSON object on stdout.

    python tools/bench_pose_graph_loops.py > profiles/pose_graph_loops.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_pose_graph import _graph, cpu_spsolve, drive  # noqa: E402
from tools.bench_raycast import alternating  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--loops", type=int, nargs="+", default=[1, 32, 128, 256, 512])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--outer", type=int, default=6)
    ap.add_argument("--max-cg", type=int, default=40000)
    ap.add_argument("--no-chain-optimize", action="store_true", help="leave out the chain route's whole optimize (the slowest part)")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_graph_loops needs the MI355X: there is no CPU path and no figure to report without it")
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
            if int(eng.lib.ovn_pose_graph_loops_bytes(n, L)) <= 0:
                out["cases"].append({"nodes": n, "loops": L, "skipped": "above this library's OVN_POSE_GRAPH_MAX_LOOPS: name a build with "
                                     "-DOVN_POSE_GRAPH_MAX_LOOPS=%d in OVN_LIB to measure beyond the cap" % L})
                print("skipped N = %d, L = %d: above the library's cap" % (n, L), file=sys.stderr, flush=True)
                continue
            PG.MAX_LOOPS = max(PG.MAX_LOOPS, L)                      # PoseGraph.optimize follows the library that is loaded
            buf = eng.pose_graph_buffers(n, e, loops=L)
            case = {"nodes": n, "loops": L, "edges": e, "routes": {}, "order_of_S": int(eng.pose_graph_loops_views(buf, n, L)["sp"])}
            eng.pose_graph_linearize(poses, fixed, ij, meas, info, ptr, lst, float("inf"), buf)
            rec = eng.pose_graph_loops_prepare(poses, ij, info, buf).cpu().numpy()
            case["record_13_14"] = [float(rec[13]), float(rec[14])]
            case["cpu_spsolve"] = cpu_spsolve(n, edges, buf["blocks"].cpu().numpy(), buf["grad"].cpu().numpy())
            vec, pre = buf["grad"].clone(), torch.zeros((n, 6), dtype=torch.float64, device=eng.device)
            prep = lambda stages: (lambda: eng.pose_graph_loops_prepare(poses, ij, info, buf, stages=stages))
            solve = lambda kind, lam, first, iters, rtol=0.0: eng.pose_graph_solve(fixed, ij, ptr, lst, buf, kind, lam, rtol, first, iters)
            fns = {"prepare": prep(7), "scan": prep(1), "assembly": prep(2), "assembly_factor": prep(6),
                   "apply_loops": lambda: eng.pose_graph_precondition(vec, buf, "loops", out=pre, node_ptr=ptr, node_edge=lst),
                   "apply_chain": lambda: eng.pose_graph_precondition(vec, buf, "chain", out=pre),
                   "loops2": lambda: solve("loops", 1e-6, 0, 2), "loops6": lambda: solve("loops", 1e-6, 0, 6),
                   "chain64": lambda: solve("chain", 0.0, 0, 64)}
            t = alternating(fns, args.warmup, args.min_ms, args.rounds)
            med = lambda k: round(t[k][0], 5)
            case["prepare_ms"] = {"all": med("prepare"), "scan": med("scan"), "assembly": med("assembly"),
                                  "factor": round(t["assembly_factor"][0] - t["assembly"][0], 5), "windows_all": t["prepare"][1]}
            case["apply_ms"] = {"loops": med("apply_loops"), "chain": med("apply_chain")}
            r6 = solve("loops", 1e-6, 0, 6).cpu().numpy()
            case["pcg_iteration_ms"] = {"loops": round((t["loops6"][0] - t["loops2"][0]) / 4, 6), "chain": round(t["chain64"][0] / 64, 6),
                                        "loops_record_after_6": [float(x) for x in r6[4:8]]}
            eng.pose_graph_loops_prepare(poses, ij, info, buf)           # the stage timings left the factor of another order of calls
            for kind in ("loops", "chain"):
                k = {}
                for key, lam in (("lam0", 0.0), ("lam1e-6", 1e-6)):
                    chunk = 8 if kind == "loops" else 64
                    torch.cuda.synchronize()
                    t0, done = time.perf_counter(), 0
                    while True:
                        r = solve(kind, lam, done, chunk, 1e-8).cpu().numpy()
                        done += chunk
                        if r[6] or r[7] or done >= args.max_cg:
                            break
                    k[key] = {"iterations": int(r[4]), "converged": bool(r[6]), "breakdown": bool(r[7]), "relative_residual": float(r[5]),
                              "solve_wall_ms": round(1e3 * (time.perf_counter() - t0), 3)}
                if kind == "loops" or not args.no_chain_optimize:
                    g = _graph(PG, eng, start, edges, Z, om)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res = g.optimize(max_iterations=args.outer, preconditioner=kind, cg_chunk=chunk, max_cg=args.max_cg)
                    torch.cuda.synchronize()
                    k["optimize"] = {"wall_s": round(time.perf_counter() - t0, 4), "outer_iterations": res.outer_iterations,
                                     "cg_iterations": res.cg_iterations, "converged": bool(res.converged), "cost_initial": res.cost_initial,
                                     "cost_final": res.cost_final, "fallbacks": g.fallbacks,
                                     "max_position_error_m": float(np.linalg.norm(res.poses[:, :3, 3] - true[:, :3, 3], axis=1).max())}
                case["routes"][kind] = k
            # one outer step of each route: what the CPU solve stands against
            case["outer_step_ms"] = {"loops": round(case["prepare_ms"]["all"] + case["routes"]["loops"]["lam0"]["solve_wall_ms"], 3),
                                     "chain": case["routes"]["chain"]["lam0"]["solve_wall_ms"],
                                     "cpu_spsolve": round(1e3 * case["cpu_spsolve"].get("seconds", float("nan")), 3)}
            out["cases"].append(case)
            print("done N = %d, L = %d: %s" % (n, L, json.dumps(case["outer_step_ms"])), file=sys.stderr, flush=True)
            del buf
            torch.cuda.empty_cache()
    eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
