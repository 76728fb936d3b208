"""One odometry track step on the rolling TSDF window against the same step on a fixed volume sized for the drive (DESIGN.md
section 36): is the window's step independent of the drive's length, and what does the ring addressing cost?

The scene is `tools/bench_render.py`'s seeded 200 m x 200 m height field; `--scans` 64 x 900 scans rendered around the field's middle
are fused into every volume, so that each holds the same surface around the sensor.  At voxel 0.2 and max_range 50 the window is the
smallest the following tracker accepts (half extent >= max_range + trunc + voxel + shift * voxel), 24 m high.  A fixed volume for a
straight drive of L metres is (L + 2 max_range) x 2 max_range x 24 m, the sensor in its middle; beyond the field it is empty space,
which is what most of a long drive's box is to any one frame.

  step             per volume -- the window, then the fixed volume for every `--drives` length -- ms per call of the stages that touch the
                   volume: fuse (one scan), bricks, raycast with the mask and without it; the window adds shift (an 8-voxel move along x
                   and back, two calls) and leaving_mesh (the cells an 8-voxel move loses, extracted and copied to the host: wall
                   time, the count is read back)
  equal_samples    the window's kernels against the dense kernels on a dense volume of the window's own shape and content, base chosen
                   so that the seam lies mid-volume on every axis: window ms / dense ms per kernel

Timing: HIP events around windows of at least `--min-ms` of device time after `--warmup` calls; the variants take turns, one window
each per round; the median and the minimum of `--rounds` rounds are reported with every window.  No threshold is set: the figures are
the result.  ONE JSON object on stdout.

    python tools/bench_tsdf_window.py > profiles/tsdf_window.json"""
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
from tools.bench_render import EXTENT, FOV_DOWN, FOV_UP, H, MAX_RANGE, SENSOR_Z, W, ground, make_mesh, make_poses  # noqa: E402

HEIGHT = 24.0
Z_LO = -4.0


def _stats(res):
    return {k: {"ms_median": round(ms, 4), "ms_min": round(min(wins), 4), "windows_ms": wins} for k, (ms, wins) in res.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=224, help="quads per side of the source height field")
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--shift", type=int, default=8)
    ap.add_argument("--drives", type=float, nargs="+", default=[100.0, 1000.0, 4000.0], help="drive lengths in metres")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_window needs the MI355X: there is no CPU path and no figure to report without it")
    from overlapnet_amd import tsdf
    from overlapnet_amd.engine import OvnEngine
    eng = OvnEngine()
    dev = eng.device
    sensor = dict(fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE)
    source = make_mesh(a.grid)
    poses = make_poses(a.scans, 1)
    mid = np.array([EXTENT / 2, EXTENT / 2])
    poses[:, :2, 3] = mid + (poses[:, :2, 3] - mid) * (4.0 / EXTENT)            # all within 2 m of the middle: one place on a drive
    poses[:, 2, 3] = ground(poses[:, 0, 3], poses[:, 1, 3]) + SENSOR_Z
    ranges = eng.render_scans(source, poses, H, W, want=("range",), **sensor)["range"]
    view = torch.from_numpy(poses[:1]).to(dev)
    trunc = tsdf.DEFAULT_TRUNC_VOXELS * a.voxel
    half = MAX_RANGE + trunc + a.voxel + a.shift * a.voxel
    try:
        clock = "%d MHz" % torch.cuda.clock_rate(0)
    except Exception as e:                                                      # noqa: BLE001 -- noted, not needed
        clock = "not available (%s)" % type(e).__name__
    out = {"device": torch.cuda.get_device_name(0), "sm_clock_at_start": clock,
           "sensor": dict(H=H, W=W, min_range=MIN_RANGE, **sensor), "voxel": a.voxel, "trunc": trunc, "shift": a.shift,
           "scans_fused": a.scans, "timing": {"warmup": a.warmup, "min_ms": a.min_ms, "rounds": a.rounds}, "step": {}}

    def stages(vol, extra):
        """The stages of a track step that touch `vol` (fused already): name -> callable."""
        scratch_t, scratch_w = vol.tsdf.clone(), vol.weight.clone()
        mask = vol.bricks()
        imgs = dict(range=torch.empty((1, H, W), device=dev), vertex=torch.empty((1, H, W, 4), device=dev),
                    normal=torch.empty((1, H, W, 3), device=dev))
        cast = lambda m: eng.tsdf_raycast(vol.tsdf, vol.weight, vol.origin, vol.voxel, view, H, W, FOV_UP, FOV_DOWN, MIN_RANGE, MAX_RANGE,
                                          vol.voxel, 1.0, m, want=(), out=imgs, **vol._window())
        fns = {"fuse": lambda: eng.tsdf_integrate(scratch_t, scratch_w, vol.origin, vol.voxel, vol.trunc, vol.max_weight, ranges[:1], view,
                                                  FOV_UP, FOV_DOWN, MAX_RANGE, **vol._window()),
               "bricks": lambda: eng.tsdf_bricks(vol.weight, 1.0, out=mask),
               "raycast": lambda: cast(mask), "raycast_no_mask": lambda: cast(None)}
        fns.update(extra(scratch_t, scratch_w))
        hits = int((cast(mask)["range"] > 0).sum().item())
        return fns, hits

    # the window, following a sensor in the field's middle
    win = tsdf.RollingTsdfVolume(eng, (2 * half, 2 * half, HEIGHT), a.voxel, anchor=(0.0, 0.0, Z_LO + HEIGHT / 2), shift=a.shift)
    win.follow(poses[0, :3, 3])
    win.integrate(ranges, poses, **sensor)
    there = tuple(b + s for b, s in zip(win.base, (a.shift, 0, 0)))

    def window_extra(scratch_t, scratch_w):
        def shift_and_back():
            eng.tsdf_window_shift(scratch_t, scratch_w, win.base, there)
            eng.tsdf_window_shift(scratch_t, scratch_w, there, win.base)
        return {"shift_there_and_back": shift_and_back}

    fns, hits = stages(win, window_extra)
    res = alternating(fns, a.warmup, a.min_ms, a.rounds)
    wall, leaving = [], 0
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        leaving = sum(int(win.triangles(box=b).cpu().shape[0]) for b in tsdf.leaving_boxes(win.base, there, tuple(n - 1 for n in win.shape)))
        wall.append((time.perf_counter() - t0) * 1e3)
    rec = {"shape": list(win.shape), "samples": win.n_samples, "base": list(win.base), "hits_of_the_view": hits, "stages": _stats(res),
           "leaving_mesh": {"triangles": leaving, "wall_ms_median": round(float(np.median(wall)), 4), "wall_ms_min": round(min(wall), 4)}}
    st = rec["stages"]
    rec["step_ms"] = {"follow_and_shift": round(st["shift_there_and_back"]["ms_median"] / 2 + rec["leaving_mesh"]["wall_ms_median"], 4),
                      "fuse": st["fuse"]["ms_median"], "bricks": st["bricks"]["ms_median"], "raycast": st["raycast"]["ms_median"],
                      "raycast_no_mask": st["raycast_no_mask"]["ms_median"]}
    out["step"]["window"] = rec
    window_hits = hits

    # the window's kernels against the dense kernels at equal sample count and content
    # the same region of space under an anchor that puts the seam mid-volume on every axis: base = n / 2, so slot 0 holds sample n
    mid_base = tuple((n // 16) * 8 for n in win.shape)
    lo = win.anchor + np.asarray(win.base) * a.voxel
    ring = tsdf.RollingTsdfVolume(eng, (2 * half, 2 * half, HEIGHT), a.voxel, anchor=lo - np.asarray(mid_base) * a.voxel, shift=a.shift)
    ring.base = mid_base                                                        # a fresh window is fresh at any base
    ring.integrate(ranges, poses, **sensor)
    dense = tsdf.TsdfVolume(eng, lo, lo + (np.asarray(ring.shape) - 1) * a.voxel, a.voxel)
    assert (dense.nx, dense.ny, dense.nz) == ring.shape, ((dense.nx, dense.ny, dense.nz), ring.shape)
    dense.integrate(ranges, poses, **sensor)
    pair = {}
    for name, vol in (("window", ring), ("dense", dense)):
        fns, hits = stages(vol, lambda t, w: {})
        cap_box = {} if name == "dense" else dict(base=ring.base, box=(ring.base, tuple(b + n - 1 for b, n in zip(ring.base, ring.shape))))
        total = eng.tsdf_triangles(vol.tsdf, vol.weight, vol.origin, vol.voxel, 1.0, capacity=0, **cap_box)[1]
        buf = torch.empty((max(total, 1), 3, 3), dtype=torch.float32, device=dev)
        fns["triangles_count_and_write"] = (lambda vol=vol, cap_box=cap_box, buf=buf:
                                            eng.tsdf_triangles(vol.tsdf, vol.weight, vol.origin, vol.voxel, 1.0, out=buf, **cap_box))
        pair[name] = (fns, hits, total)
    both = {"%s_%s" % (n, k): f for n in pair for k, f in pair[n][0].items()}
    res = alternating(both, a.warmup, a.min_ms, a.rounds)
    eq = {"shape": list(ring.shape), "samples": ring.n_samples, "window_base": list(ring.base),
          "hits": {n: pair[n][1] for n in pair}, "triangles": {n: pair[n][2] for n in pair}, "kernels": {}}
    for k in pair["window"][0]:
        wn, dn = res["window_" + k], res["dense_" + k]
        eq["kernels"][k] = {"window": _stats({k: wn})[k], "dense": _stats({k: dn})[k], "window_over_dense_median": round(wn[0] / dn[0], 4),
                            "window_over_dense_min": round(min(wn[1]) / min(dn[1]), 4)}
    out["equal_samples"] = eq
    del ring, dense, pair, both
    torch.cuda.empty_cache()

    # the fixed volume of the parent route, sized for a drive of L metres
    for L in a.drives:
        lo = np.array([mid[0] - L / 2 - MAX_RANGE, mid[1] - MAX_RANGE, Z_LO])
        hi = np.array([mid[0] + L / 2 + MAX_RANGE, mid[1] + MAX_RANGE, Z_LO + HEIGHT])
        try:
            vol = tsdf.TsdfVolume(eng, lo, hi, a.voxel)
        except ValueError as e:
            out["step"]["fixed_%gm" % L] = {"refused": str(e)}
            continue
        vol.integrate(ranges, poses, **sensor)
        fns, hits = stages(vol, lambda t, w: {})
        res = alternating(fns, a.warmup, a.min_ms, a.rounds)
        st = _stats(res)
        out["step"]["fixed_%gm" % L] = {
            "shape": [vol.nx, vol.ny, vol.nz], "samples": vol.n_samples, "gigabytes": round(vol.n_samples * 8 / 1e9, 3),
            "hits_of_the_view": hits, "same_hits_as_the_window": hits == window_hits, "stages": st,
            "step_ms": {k: st[k]["ms_median"] for k in ("fuse", "bricks", "raycast", "raycast_no_mask")}}
        del vol, fns
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
