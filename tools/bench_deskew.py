"""Throughput of `ovn_deskew` (csrc/deskew.hip) and what it adds to a `TsdfOdometry.track` frame.

  deskew     1, 64 and 1024 scans of `--points` points each (120 000: a 64-beam sensor's sweep), by per-point times and by azimuth:
             ms per call, points per second, and the bytes per second of the traffic the kernel needs (16 in + 16 out per point, + 4
             of a given time).  The yardstick is measured in the same run, taking turns with the kernel: a `torch` copy of the same
             points, which moves 32 bytes per point and does nothing else
  track      a tracker's frame on a straight drive through `tools/bench_render.py`'s height field, with deskew off, on (one pass)
             and on with two passes: wall milliseconds per `track` call, the variants taking turns frame by frame on trackers of
             their own.  The scans are snapshots, so the three see the same points; what differs is the work

Timing: HIP events around windows of at least `--min-ms` of device time, the median of `--rounds` rounds with every window reported
(`tools/bench_raycast.py`'s `alternating`).  No threshold is set and no figure is promised: a record for a later reader.

    python tools/bench_deskew.py            # writes profiles/deskew.json (--out), and prints the same JSON object"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_raycast import MIN_RANGE, alternating  # noqa: E402
from tools.bench_render import FOV_DOWN, FOV_UP, H, MAX_RANGE, SENSOR_Z, W, ground, make_mesh  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=120000, help="points per scan")
    ap.add_argument("--scans", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--grid", type=int, default=224, help="quads per side of the height field the tracked drive runs through")
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--track-frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_deskew needs the MI355X: there is no CPU path and no figure to report without it")
    from overlapnet_amd import odometry
    from overlapnet_amd.deskew import deskew_scans
    from overlapnet_amd.engine import OvnEngine
    eng = OvnEngine()
    dev = eng.device
    out = {"device": torch.cuda.get_device_name(0), "points_per_scan": a.points, "deskew": {}}
    g = torch.Generator(device="cpu").manual_seed(1)
    for n in a.scans:
        total = n * a.points
        pts = ((torch.rand((total, 4), generator=g) - 0.5) * 80.0).to(dev)
        times = torch.rand(total, generator=g).to(dev)
        offs = torch.arange(0, total + 1, a.points, dtype=torch.int64, device=dev)
        tw = torch.cat([torch.rand((n, 3), generator=g, dtype=torch.float64), 0.05 * torch.rand((n, 3), generator=g, dtype=torch.float64)], 1).to(dev)
        res, copy = torch.empty_like(pts), torch.empty_like(pts)
        fns = {"times": lambda: deskew_scans(eng, pts, offs, tw, times=times, out=res),
               "azimuth": lambda: deskew_scans(eng, pts, offs, tw, start_azimuth=-180.0, clockwise=True, out=res),
               "torch_copy": lambda: copy.copy_(pts)}
        rec = {"points": total}
        for k, (ms, wins) in alternating(fns, a.warmup, a.min_ms, a.rounds).items():
            per_point = {"times": 36, "azimuth": 32, "torch_copy": 32}[k]
            rec[k] = {"ms_per_call": round(ms, 5), "windows_ms": wins, "points_per_s": total / (ms * 1e-3),
                      "bytes_per_point": per_point, "bytes_per_s": total * per_point / (ms * 1e-3)}
        for k in ("times", "azimuth"):
            rec[k]["time_over_torch_copy"] = round(rec[k]["ms_per_call"] / rec["torch_copy"]["ms_per_call"], 3)
        out["deskew"]["%d_scans" % n] = rec
        del pts, times, res, copy
        torch.cuda.empty_cache()

    # a tracker's frame with and without deskew: a straight drive of 0.5 m per frame, rendered as snapshots
    n = a.track_frames
    sensor = dict(fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE)
    drive = np.tile(np.eye(4), (n, 1, 1))
    drive[:, 0, 3] = 60.0 + 0.5 * np.arange(n)
    drive[:, 1, 3] = 112.0
    drive[:, 2, 3] = ground(drive[:, 0, 3], drive[:, 1, 3]) + SENSOR_Z
    rel = np.linalg.inv(drive[0])[None] @ drive
    rr = eng.render_scans(make_mesh(a.grid), drive, H, W, want=("range", "vertex"), **sensor)
    rng_h, vtx_h = rr["range"].cpu().numpy(), rr["vertex"].cpu().numpy()
    clouds = [torch.from_numpy(np.ascontiguousarray(vtx_h[s][rng_h[s] > 0], np.float32)).to(dev) for s in range(n)]
    blo, bhi = odometry.bounds_from_poses(rel, MAX_RANGE)
    azimuth = dict(start_azimuth=-180.0, clockwise=True)
    variants = {"off": {}, "on_1_pass": dict(deskew=azimuth, deskew_passes=1), "on_2_passes": dict(deskew=azimuth, deskew_passes=2)}
    trackers = {k: odometry.TsdfOdometry(eng, blo, bhi, a.voxel, proj_h=H, proj_w=W, min_range=MIN_RANGE, **sensor, **kw)
                for k, kw in variants.items()}
    wall = {k: [] for k in variants}
    for c in clouds:
        for k, odo in trackers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            odo.track(c)
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    out["track"] = {"frames": n, "points_per_scan": [int(c.shape[0]) for c in clouds], "image": [H, W],
                    "volume": [trackers["off"].volume.nx, trackers["off"].volume.ny, trackers["off"].volume.nz],
                    "note": "frames 0 and 1 deskew nothing; frame 2 of a deskewing tracker also rebuilds the model from scans 0 and 1",
                    "wall_ms": {k: [round(x, 3) for x in v] for k, v in wall.items()},
                    "wall_ms_median_from_frame_3": {k: round(float(np.median(v[3:])), 3) for k, v in wall.items()},
                    "last_frame_translation_error_m": {k: float(np.linalg.norm(o.poses[-1][:3, 3] - rel[-1][:3, 3]))
                                                       for k, o in trackers.items()}}
    text = json.dumps(out, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
