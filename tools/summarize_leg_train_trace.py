#!/usr/bin/env python3
"""Per-kernel split of tools/bench_leg_train.py from its `rocprofv3 --kernel-trace --stats` run (the rocpd sqlite output) into
profiles/leg_train_kernels.{md,json}.

    rocprofv3 --kernel-trace --stats -d trace_out/leg_train -o leg_train -- python tools/bench_leg_train.py --skip-trainer --skip-torch
    python tools/summarize_leg_train_trace.py trace_out/leg_train"""
import glob
import json
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.summarize_rocprof import short  # noqa: E402


def main():
    src = sys.argv[1]
    dbs = sorted(glob.glob(os.path.join(src, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit("no rocpd database under %s" % src)
    con = sqlite3.connect(dbs[0])
    rows = con.execute("select name,total_calls,total_duration,average,percentage from top_kernels").fetchall()
    lines = ["# rocprofv3 --kernel-trace --stats of tools/bench_leg_train.py --skip-trainer --skip-torch", "",
             "All dispatches of the run, warm-up included (durations in us).", "", "| kernel | calls | total us | avg us | % |",
             "|---|---|---|---|---|"]
    out = {"kernels": []}
    for name, calls, tot, avg, pct in rows:
        out["kernels"].append({"name": short(name), "calls": calls, "total_us": tot, "avg_us": avg, "pct": pct})
        lines.append("| `%s` | %d | %.1f | %.2f | %.2f |" % (short(name), calls, tot, avg, pct))
    dst = os.path.join(ROOT, "profiles")
    with open(os.path.join(dst, "leg_train_kernels.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(dst, "leg_train_kernels.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
