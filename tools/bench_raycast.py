"""Throughput of `ovn_tsdf_raycast` / `ovn_tsdf_bricks` (csrc/tsdf_raycast.hip), the route they replace for a view of a volume that
has just changed, and one `TsdfOdometry.track` step split into its stages.

The scene is `tools/bench_tsdf.py`'s: the seeded 200 m x 200 m height field, `--scans` 64 x 900 scans rendered from it and fused into
the volume over the whole field at voxel 0.2 (1001 x 1001 x 121 = 121 M samples).  Timing: HIP events around windows of at least
`--min-ms` of device time; the variants of one comparison (with and without the brick mask) take turns, one window each per round, and
the median of `--rounds` rounds is reported with every window (bench_render's `window`, alternating).

  raycast        one 64 x 900 view and 64 views, with the mask and without: ms per call, rays per second, hits, samples marched per
                 ray (from the hit ranges: a missing ray marches all K)
  bricks         ms of the mask itself (the odometry rebuilds it every frame)
  replaced_route the same one view through the mesh: `vol.mesh()` (two extraction calls and the copy to the host), the host-side
                 hierarchy build, `render_scans` of one pose -- wall seconds, since most of it is host work
  track_step     project, mask, ray-cast with and without it, register (both pairs, one launch), fuse: ms per call each, on the
                 odometry's own buffers after `--track-frames` tracked frames of a straight drive; and the wall time of whole `track`
                 calls (which run without the mask, the tracker's default)

No figure is promised; ONE JSON object on stdout.

    python tools/bench_raycast.py > profiles/tsdf_raycast.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_render import EXTENT, FOV_DOWN, FOV_UP, H, MAX_RANGE, SENSOR_Z, W, ground, make_mesh, make_poses  # noqa: E402

Z_LO, Z_HI = -4.0, 20.0
MIN_RANGE = 0.5


def alternating(fns, warmup, min_ms, rounds):
    """name -> (median ms per call, the windows): per round one window of at least min_ms of device time for every variant in turn."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            calls = 0
            a.record()
            while True:
                fn()
                calls += 1
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                if ms >= min_ms:
                    break
            per[k].append(ms / calls)
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in per.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=224, help="quads per side of the source height field")
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--track-frames", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_raycast needs the MI355X: there is no CPU path and no figure to report without it")
    from overlapnet_amd import odometry, tsdf
    from overlapnet_amd.engine import OvnEngine
    eng = OvnEngine()
    sensor = dict(fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE)
    source = make_mesh(a.grid)
    poses = make_poses(a.scans, 1)
    r = eng.render_scans(source, poses, H, W, want=("range", "vertex"), **sensor)
    lo, hi = np.array([0.0, 0.0, Z_LO]), np.array([EXTENT, EXTENT, Z_HI])
    vol = tsdf.TsdfVolume(eng, lo, hi, a.voxel)
    vol.integrate(r["range"], poses, **sensor)
    K = tsdf.check_march(MIN_RANGE, MAX_RANGE, vol.voxel)
    out = {"sensor": dict(H=H, W=W, min_range=MIN_RANGE, **sensor), "device": torch.cuda.get_device_name(0), "scans_fused": a.scans,
           "volume": {"shape": [vol.nx, vol.ny, vol.nz], "samples": vol.n_samples, "voxel": vol.voxel, "trunc": vol.trunc},
           "samples_per_ray_K": K}
    mask = vol.bricks()
    out["volume"]["live_bricks"] = int(mask.sum().item())
    out["volume"]["bricks"] = int(mask.numel())
    views = make_poses(64, 2)                                   # other poses than the fused ones
    d_views = torch.from_numpy(views).to(eng.device)
    cast = lambda p, m: eng.tsdf_raycast(vol.tsdf, vol.weight, vol.origin, vol.voxel, p, H, W, FOV_UP, FOV_DOWN, MIN_RANGE, MAX_RANGE,
                                         vol.voxel, 1.0, m, want=("range", "normal"))
    out["raycast"] = {}
    for name, p in (("one_view", d_views[:1]), ("64_views", d_views)):
        res = alternating({"mask": lambda: cast(p, mask), "no_mask": lambda: cast(p, None)}, a.warmup, a.min_ms, a.rounds)
        rng = cast(p, mask)["range"]
        same = torch.equal(rng.view(torch.int32), cast(p, None)["range"].view(torch.int32))
        hit = rng > 0
        marched = torch.where(hit, torch.ceil((rng - MIN_RANGE) / vol.voxel) + 1.0, torch.full_like(rng, float(K)))
        rays = int(rng.numel())
        rec = {"rays": rays, "hit_share": float(hit.float().mean().item()), "samples_marched_per_ray": float(marched.mean().item()),
               "mask_route_has_the_null_route_bits": bool(same)}
        for k, (ms, wins) in res.items():
            rec[k] = {"ms_per_call": round(ms, 4), "windows_ms": wins, "rays_per_s": rays / (ms * 1e-3),
                      "samples_per_s": rays * rec["samples_marched_per_ray"] / (ms * 1e-3)}
        out["raycast"][name] = rec
    ms, wins = alternating({"bricks": lambda: eng.tsdf_bricks(vol.weight, 1.0, out=mask)}, a.warmup, a.min_ms, a.rounds)["bricks"]
    out["bricks"] = {"ms_per_call": round(ms, 4), "windows_ms": wins, "weight_bytes_per_s": vol.n_samples * 4 / (ms * 1e-3)}

    # the route a changed volume takes without the ray caster: extract, copy, build the hierarchy on the host, render
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = vol.mesh()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mesh.bvh
        t2 = time.perf_counter()
        eng.render_scans(mesh, views[:1], H, W, want=("range", "normal"), **sensor)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        runs.append({"mesh_s": round(t1 - t0, 4), "bvh_build_host_s": round(t2 - t1, 4), "upload_and_render_s": round(t3 - t2, 4),
                     "total_s": round(t3 - t0, 4)})
        triangles = mesh.n_triangles
        del mesh
    total = float(np.median([x["total_s"] for x in runs]))
    one = out["raycast"]["one_view"]
    out["replaced_route"] = {"triangles": triangles, "runs": runs, "total_s": round(total, 4),
                             "over_mask_plus_one_masked_view": total / ((out["bricks"]["ms_per_call"] + one["mask"]["ms_per_call"]) * 1e-3)}
    del vol, mask
    torch.cuda.empty_cache()

    # one track step on a drive along x through the field's middle, split into the calls `TsdfOdometry.track` makes
    n = a.track_frames + 1
    drive = np.tile(np.eye(4), (n, 1, 1))
    drive[:, 0, 3] = 60.0 + 0.5 * np.arange(n)
    drive[:, 1, 3] = 112.0
    drive[:, 2, 3] = ground(drive[:, 0, 3], drive[:, 1, 3]) + SENSOR_Z
    rel = np.linalg.inv(drive[0])[None] @ drive
    rr = eng.render_scans(source, drive, H, W, want=("range", "vertex"), **sensor)
    rng_h, vtx_h = rr["range"].cpu().numpy(), rr["vertex"].cpu().numpy()
    clouds = [np.ascontiguousarray(vtx_h[s][rng_h[s] > 0], np.float32) for s in range(n)]
    blo, bhi = odometry.bounds_from_poses(rel, MAX_RANGE)
    odo = odometry.TsdfOdometry(eng, blo, bhi, a.voxel, proj_h=H, proj_w=W, min_range=MIN_RANGE, **sensor)
    wall = []
    for c in clouds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = odo.track(c)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    err = float(np.linalg.norm(res.pose[:3, 3] - rel[-1][:3, 3]))
    v = odo.volume
    pts = torch.from_numpy(clouds[-1]).to(eng.device)
    offs = torch.tensor([0, pts.shape[0]], dtype=torch.int64, device=eng.device)
    pose_dev = torch.from_numpy(res.pose[None]).to(eng.device)
    bm = eng.tsdf_bricks(v.weight, 1.0)
    scratch_t, scratch_w = v.tsdf.clone(), v.weight.clone()
    stages = {
        "project": lambda: eng.project(pts, offs, int(pts.shape[0]), H, W, FOV_UP, FOV_DOWN, MAX_RANGE, want=("range", "vertex", "normal")),
        "mask": lambda: eng.tsdf_bricks(v.weight, 1.0, out=bm),
        "raycast": lambda: eng.tsdf_raycast(v.tsdf, v.weight, v.origin, v.voxel, pose_dev, H, W, FOV_UP, FOV_DOWN, MIN_RANGE, MAX_RANGE,
                                            v.voxel, 1.0, bm, want=(),
                                            out=dict(range=odo.range[0:1], vertex=odo.vertex[0:1], normal=odo.normal[0:1])),
        "raycast_no_mask": lambda: eng.tsdf_raycast(v.tsdf, v.weight, v.origin, v.voxel, pose_dev, H, W, FOV_UP, FOV_DOWN, MIN_RANGE,
                                                    MAX_RANGE, v.voxel, 1.0, None, want=(),
                                                    out=dict(range=odo.range[0:1], vertex=odo.vertex[0:1], normal=odo.normal[0:1])),
        "register": lambda: eng.icp_register(odo.vertex, odo.normal, odo.range, odo._src, odo._tgt, odo._init, **sensor),
        "fuse": lambda: eng.tsdf_integrate(scratch_t, scratch_w, v.origin, v.voxel, v.trunc, v.max_weight, odo.range[1:2], pose_dev,
                                           FOV_UP, FOV_DOWN, MAX_RANGE)}
    res_st = alternating(stages, a.warmup, a.min_ms, a.rounds)
    out["track_step"] = {"volume": [v.nx, v.ny, v.nz], "samples": v.n_samples, "frames_tracked": n,
                         "sources": [x.source for x in odo.results], "last_frame_translation_error_m": err,
                         "track_wall_s": [round(x, 4) for x in wall], "track_wall_s_median_after_first": round(float(np.median(wall[1:])), 4),
                         "stages": {k: {"ms_per_call": round(ms, 4), "windows_ms": wins} for k, (ms, wins) in res_st.items()},
                         "step_with_mask_ms": round(sum(res_st[k][0] for k in ("project", "mask", "raycast", "register", "fuse")), 4),
                         "step_without_mask_ms": round(sum(res_st[k][0] for k in ("project", "raycast_no_mask", "register", "fuse")), 4)}
    print(json.dumps(out, indent=1))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
