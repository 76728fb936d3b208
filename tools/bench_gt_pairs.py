"""Labelling every frame of a sequence against every scan: the loop of `OverlapGroundTruth.mapping(f)` (path a: per frame N range
images through fill / scatter / finish / count, N yaw bins with one inversion each) against `mapping_all()` (path b: one pair
kernel per pass, `yaw_bins_all`), in ONE run on the same object.

Inputs: N in {16, 256} scans, the two fixture scans alternating, under seeded poses along a curved track with straight stretches
(same-rotation neighbours: the yaw-bin boundary case).  Per N: `--warmup` untimed + `--reps` timed repetitions of each path,
alternating, wall clock around a device synchronise; path b starts every repetition without its cached own range images and
inverses.  The GPU part (`overlaps(f)` loop / the pair counts) and the yaw part are timed on their own in the same way.  The tool
asserts that path b returns path a's array.  Also timed with HIP events: the pair kernel alone in both workgroup orders
(OVN_GT_PAIR_ORDER).  Output: ONE JSON object on stdout.

    python tools/bench_gt_pairs.py > profiles/gt_pairs.json

`--trace N` runs each path once at N scans after one warm-up and nothing else: the workload for a run of its own under
`rocprofv3 --kernel-trace --stats -d trace_out/gt_pairs -o gt_pairs -- python tools/bench_gt_pairs.py --trace 256`;
`--summarize trace_out/gt_pairs --trace 256` then prints the us per pair of the pair kernel beside the four kernels of path a."""
import argparse
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OLD_KERNELS = ("gt_fill_kernel", "gt_scatter_kernel", "gt_finish_kernel", "gt_count_kernel")


def track_poses(n, seed=0):
    """A drive of n frames, 1 m apart: straight stretches (identical rotation), arcs of 3 degrees per frame, a little noise
    in z / pitch on the arcs."""
    rng = np.random.default_rng(seed)
    poses, yaw, pos = [], 0.0, np.zeros(3)
    for i in range(n):
        straight = (i // 8) % 2 == 0
        if not straight:
            yaw += np.radians(3.0)
        pitch = 0.0 if straight else rng.normal(0, 0.002)
        cz, sz, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        T = np.eye(4)
        T[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
        pos = pos + np.array([cz, sz, 0.0]) + (0 if straight else rng.normal(0, 0.01, 3))
        T[:3, 3] = pos
        poses.append(T)
    return np.stack(poses)


def make_gt(n):
    from tools import synthetic as S
    from overlapnet_amd.ground_truth import OverlapGroundTruth
    fx = S.load_fixture_images()
    return OverlapGroundTruth([fx["points_%d" % (i % 2)] for i in range(n)], track_poses(n))


def _forget(gt):
    gt._cur = gt._valid = gt._inv_poses = None


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3)}


def paths(gt):
    from overlapnet_amd.ground_truth import yaw_bin, yaw_bins_all
    n = gt.n
    everything = np.arange(n)

    def b_gpu():
        _forget(gt)
        return gt._pair_counts(everything, None, None)

    def b_total():
        _forget(gt)
        return gt.mapping_all()

    return {
        "a_total": lambda: np.concatenate([gt.mapping(f) for f in range(n)]),
        "b_total": b_total,
        "a_gpu": lambda: [gt.overlaps(f) for f in range(n)],
        "b_gpu": b_gpu,
        "a_yaw": lambda: [[yaw_bin(gt.poses[f], gt.poses[r], gt.leg_output_width) for r in range(n)] for f in range(n)],
        "b_yaw": lambda: yaw_bins_all(gt.poses, None, None, gt.leg_output_width),
    }


def kernel_orders(gt, reps):
    """ms of one pair-kernel launch over all n x n pairs in both workgroup orders (HIP events, median of reps)."""
    import torch
    e = gt.engine
    cur, _ = gt._own_ranges(np.arange(gt.n))
    gt._pair_counts(np.arange(gt.n), None, None)
    out = {}
    results = {}
    for order in ("frame", "ref"):
        os.environ["OVN_GT_PAIR_ORDER"] = order
        ms = []
        for i in range(reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            c = e.gt_pair_counts(gt._points, gt._offsets, gt._ref_poses, gt._inv_poses, cur, fov_up=gt.proj["fov_up"],
                                 fov_down=gt.proj["fov_down"], max_range=gt.proj["max_range"])
            b.record()
            b.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        results[order] = c.cpu().numpy()
        out[order + "_fastest"] = dict(_stats(ms), us_per_pair=round(float(np.median(ms)) * 1e3 / (gt.n * gt.n), 4))
    os.environ.pop("OVN_GT_PAIR_ORDER")
    assert np.array_equal(results["frame"], results["ref"])
    return out


def summarize(src, n):
    dbs = sorted(glob.glob(os.path.join(src, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit("no rocpd database under %s" % src)
    rows = sqlite3.connect(dbs[0]).execute("select name,total_calls,total_duration from top_kernels").fetchall()
    pairs = 2 * n * n                                            # warm-up + the traced repetition of each path
    out = {"tool": "tools/bench_gt_pairs.py --summarize", "n_scans": n, "pairs_per_path": pairs, "kernels": {}}
    for name, calls, total in rows:
        for k in OLD_KERNELS + ("gt_pair_kernel",):
            if k in name:
                out["kernels"][k] = {"calls": calls, "total_us": round(total, 1), "us_per_pair": round(total / pairs, 4)}
    # the own range images of path b (n scans per repetition) run through fill / scatter / finish too: they are part of path b's
    # cost and appear in the old kernels' totals, so the old sum below is an upper bound of path a's by n / n^2
    out["old_kernels_us_per_pair"] = round(sum(out["kernels"][k]["us_per_pair"] for k in OLD_KERNELS if k in out["kernels"]), 4)
    out["pair_kernel_us_per_pair"] = out["kernels"].get("gt_pair_kernel", {}).get("us_per_pair")
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0, metavar="N")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.trace or 256)
    import torch
    torch.cuda.set_device(0)
    if a.trace:
        gt = make_gt(a.trace)
        p = paths(gt)
        for _ in range(2):
            ma, mb = p["a_total"](), p["b_total"]()
        torch.cuda.synchronize()
        assert np.array_equal(ma, mb)
        return
    rows = []
    for n in a.sizes:
        gt = make_gt(n)
        p = paths(gt)
        times = {k: [] for k in p}
        for i in range(a.warmup + a.reps):
            res = {}
            for k, fn in p.items():
                ms, res[k] = _wall(fn)
                if i >= a.warmup:
                    times[k].append(ms)
            assert np.array_equal(res["a_total"], res["b_total"]), "mapping_all differs from the loop of mapping(f)"
            assert np.array_equal(np.asarray(res["a_yaw"]), res["b_yaw"])
        row = {"n_scans": n, "pairs": n * n, "points_per_scan": int(gt.max_points)}
        row.update({k: _stats(v) for k, v in times.items()})
        row["b_slowest_below_a_fastest"] = bool(row["b_total"]["max_ms"] < row["a_total"]["min_ms"])
        row["speedup_median"] = round(row["a_total"]["median_ms"] / row["b_total"]["median_ms"], 2)
        row["pair_kernel"] = kernel_orders(gt, a.reps)
        rows.append(row)
        gt.engine.close()
    print(json.dumps({"tool": "tools/bench_gt_pairs.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
                      "warmup": a.warmup, "method": "wall clock around a device synchronise, paths alternating in one process; "
                      "pair_kernel: HIP events around one launch", "rows": rows}, indent=1))


if __name__ == "__main__":
    main()
