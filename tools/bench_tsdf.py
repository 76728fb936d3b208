"""Throughput of `ovn_tsdf_integrate` / `ovn_tsdf_triangles` (csrc/tsdf.hip) and of `OverlapMap.from_mesh` on the fused mesh.

The scene is `tools/bench_render.py`'s seeded 200 m x 200 m height field (about 10^5 triangles); `--scans` 64 x 900 scans are rendered
from it at random poses and fused into a volume over the whole field at each `--voxel` size.  Timing: `--warmup` untimed calls, then
calls between two HIP events until `--min-ms` of device time have passed, the median of `--rounds` such windows (bench_render's
`window`).  Per volume:

  integration  ms per call of the whole batch; sample-scan PAIRS per second (the pairs inside the scans' boxes, which is what the
               kernel evaluates: counted on the host with the kernel's own box rule) and the updates among them that pass every test
               (the sum of the weights after one call on a fresh volume).  Fusing again into the fused volume is the same work.
               Also one scan alone and one pose 10 km away: the grid covers the volume, so the second is what that costs by itself.
  extraction   the counting call alone (pass 1 + the scan of the workgroup counts), the writing call (pass 1 + scan + pass 2), their
               difference as the write, and the triangles out.
  torch        the same statement in plain batched torch: integration scan by scan on the box of each scan (sliced views; atan2 /
               asin are torch's own, so pixels may differ in the last bit -- this is a timing baseline, not a parity check);
               extraction up to where a torch implementation could start writing: the per-cell triangle counts and their cumsum.
  limits       bytes and float operations per pair / per cell COUNTED from the kernels' code (the constants below), over the HBM and
               the fp32 vector peak.

Then `OverlapMap.from_mesh` on `--map-poses` grid poses with test weights, on the source mesh and on the mesh fused at the first voxel
size: wall seconds of the whole call.  ONE JSON object on stdout.

    python tools/bench_tsdf.py > profiles/tsdf.json"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_render import EXTENT, FOV_DOWN, FOV_UP, H, MAX_RANGE, SENSOR_Z, W, ground, make_mesh, make_poses, window  # noqa: E402

HBM_PEAK, FP32_PEAK = 8.0e12, 157.3e12          # bytes/s and FLOP/s (spec)
Z_LO, Z_HI = -4.0, 20.0
# counted from tsdf_integrate_kernel: per sample and call 8 B read + 8 B written; per pair 3 sub + 9 mul + 6 add (R^T d), 5 + sqrt
# (depth), the two SVML functions (atan2f_np 38, asinf_np 29 float operations on their main paths, svml_f32.h), 10 for px / py and the
# tests, 7 for sdf .. weight, and one 4-byte gather from the scan's range image (230 KB: L2)
SAMPLE_BYTES, PAIR_FLOPS, PAIR_GATHER_BYTES = 16, 18 + 6 + 38 + 29 + 10 + 7, 4
# counted from tsdf_cells_kernel: per cell 8 tsdf + 8 weight loads of 4 B, of which 4 B + 4 B are new to the cache hierarchy (a sample is
# a corner of eight cells); per triangle 36 B written and 6 corner reloads that hit L1 / L2
CELL_BYTES_HBM, TRIANGLE_BYTES = 8, 36


def box_pairs(poses, origin, shape, voxel, trunc, max_range):
    """Samples inside the box of every scan (tsdf_prepare_kernel's rule), summed: the pairs the kernel evaluates."""
    reach = (max_range + trunc) + voxel
    total = 0
    for p in poses:
        n = 1
        for a in range(3):
            lo = max(0.0, np.floor((p[a, 3] - reach - origin[a]) / voxel) - 1.0)
            hi = min(shape[a] - 1.0, np.ceil((p[a, 3] + reach - origin[a]) / voxel) + 1.0)
            n *= max(0.0, hi - lo + 1.0)
        total += n
    return int(total)


def torch_integrate(tsdf, weight, origin, voxel, trunc, max_weight, rng, poses, max_range):
    """The statement of ovn_tsdf_integrate in batched float32 torch, one scan at a time on that scan's box."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    n, h, w = rng.shape
    up, down = FOV_UP / 180.0 * np.pi, FOV_DOWN / 180.0 * np.pi
    fda, fov = float(np.float32(abs(down))), float(np.float32(abs(down) + abs(up)))
    reach = (max_range + trunc) + voxel
    P = torch.as_tensor(poses, dtype=torch.float32, device=dev)
    for s in range(n):
        sl = []
        for a, dim in enumerate((nx, ny, nz)):
            lo = int(max(0.0, np.floor((poses[s][a, 3] - reach - origin[a]) / voxel) - 1.0))
            hi = int(min(dim - 1.0, np.ceil((poses[s][a, 3] + reach - origin[a]) / voxel) + 1.0))
            sl.append(slice(lo, hi + 1))
        if any(x.stop <= x.start for x in sl):
            continue
        t, wt = tsdf[sl[2], sl[1], sl[0]], weight[sl[2], sl[1], sl[0]]
        ax = [float(np.float32(origin[a])) + torch.arange(sl[a].start, sl[a].stop, device=dev, dtype=torch.float32) * float(np.float32(voxel))
              for a in range(3)]
        d = [ax[0][None, None, :] - P[s, 0, 3], ax[1][None, :, None] - P[s, 1, 3], ax[2][:, None, None] - P[s, 2, 3]]
        q = [(P[s, 0, c] * d[0] + P[s, 1, c] * d[1]) + P[s, 2, c] * d[2] for c in range(3)]
        depth = torch.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        yaw = -torch.atan2(q[1], q[0])
        pitch = torch.asin(q[2] / depth)
        px = (0.5 * (yaw / float(np.float32(np.pi)) + 1.0)) * float(w)
        py = (1.0 - (pitch + fda) / fov) * float(h)
        ok = (depth > 0) & (py >= 0) & (py < float(h))
        col = torch.clamp(torch.floor(px), 0, w - 1).long()
        row = torch.where(ok, torch.floor(py), torch.zeros_like(py)).long()
        r = rng[s][row, col]
        sdf = r - depth
        ok = ok & (r > 0) & (r < max_range) & ~(sdf < -trunc)
        dv = torch.clamp(sdf / trunc, max=1.0)
        w1 = wt + 1.0
        t.copy_(torch.where(ok, (wt * t + dv) / w1, t))
        wt.copy_(torch.where(ok, torch.clamp(w1, max=max_weight), wt))


TETS = ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7))


def torch_count(tsdf, weight, min_weight):
    """Per-cell triangle counts of the marching tetrahedra and their exclusive offsets: what a torch extraction needs before it writes."""
    nz, ny, nx = tsdf.shape
    corner = lambda a, c: a[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    inside = [corner(tsdf, c) < 0 for c in range(8)]
    seen = corner(weight, 0) >= min_weight
    for c in range(1, 8):
        seen = seen & (corner(weight, c) >= min_weight)
    count = torch.zeros_like(inside[0], dtype=torch.int32)
    for tet in TETS:
        k = inside[tet[0]].to(torch.int32) + inside[tet[1]].to(torch.int32) + inside[tet[2]].to(torch.int32) + inside[tet[3]].to(torch.int32)
        count += torch.where(k == 2, 2, ((k == 1) | (k == 3)).to(torch.int32))
    count = torch.where(seen, count, torch.zeros_like(count)).reshape(-1)
    offsets = torch.cumsum(count, 0, dtype=torch.int64) - count
    return int(count.sum().item()), offsets


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=224, help="quads per side of the source height field")
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--voxel", type=float, nargs="+", default=[0.4, 0.2], help="one volume over the whole field per voxel size")
    ap.add_argument("--map-poses", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs the MI355X: there is no CPU path and no figure to report without it")
    from tools import synthetic as S
    from overlapnet_amd import tsdf
    from overlapnet_amd.infer import FeatureVolumeCache, Infer
    from overlapnet_amd.localization import OverlapMap, grid_poses
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[H, W]), "infer_seqs": "07", "data_root_folder": tempfile.mkdtemp(),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    infer = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    eng = infer.engine
    sensor = dict(fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE)
    source = make_mesh(a.grid)
    poses = make_poses(a.scans, 1)
    rng = eng.render_scans(source, poses, H, W, want=("range",), **sensor)["range"]
    out = {"sensor": dict(H=H, W=W, **sensor), "device": torch.cuda.get_device_name(0), "scans": a.scans,
           "source_triangles": source.n_triangles, "peaks": {"hbm_bytes_per_s": HBM_PEAK, "fp32_vector_flop_per_s": FP32_PEAK},
           "counted_from_the_code": {"bytes_per_sample_and_call": SAMPLE_BYTES, "flop_per_pair": PAIR_FLOPS,
                                     "gather_bytes_per_pair": PAIR_GATHER_BYTES, "hbm_bytes_per_cell": CELL_BYTES_HBM,
                                     "bytes_per_triangle": TRIANGLE_BYTES}, "volumes": []}
    lo, hi = np.array([0.0, 0.0, Z_LO]), np.array([EXTENT, EXTENT, Z_HI])
    fused_mesh = None
    for voxel in a.voxel:
        vol = tsdf.TsdfVolume(eng, lo, hi, voxel, max_weight=1.0e9)
        shape = (vol.nx, vol.ny, vol.nz)
        pairs = box_pairs(poses, vol.origin, shape, vol.voxel, vol.trunc, MAX_RANGE)
        vol.integrate(rng, poses, **sensor)
        updates = float(vol.weight.sum(dtype=torch.float64).item())
        fuse = lambda: eng.tsdf_integrate(vol.tsdf, vol.weight, vol.origin, vol.voxel, vol.trunc, vol.max_weight, rng, poses, FOV_UP,
                                          FOV_DOWN, MAX_RANGE)
        ms_int, win_int = window(fuse, a.warmup, a.min_ms, a.rounds)
        # the grid covers the volume, not the union of the batch's boxes: one scan alone (most waves end at the union test), and one
        # pose 10 km away (every wave ends there: what the whole-volume grid costs by itself)
        one = lambda: eng.tsdf_integrate(vol.tsdf, vol.weight, vol.origin, vol.voxel, vol.trunc, vol.max_weight, rng[:1], poses[:1],
                                         FOV_UP, FOV_DOWN, MAX_RANGE)
        away = poses[:1].copy()
        away[0, 0, 3] += 1.0e4
        blind = lambda: eng.tsdf_integrate(vol.tsdf, vol.weight, vol.origin, vol.voxel, vol.trunc, vol.max_weight, rng[:1], away, FOV_UP,
                                           FOV_DOWN, MAX_RANGE)
        ms_one, _ = window(one, a.warmup, a.min_ms, a.rounds)
        ms_blind, _ = window(blind, a.warmup, a.min_ms, a.rounds)
        pairs_one = box_pairs(poses[:1], vol.origin, shape, vol.voxel, vol.trunc, MAX_RANGE)
        vol.reset()
        vol.integrate(rng, poses, **sensor)
        count_only = lambda: eng.tsdf_triangles(vol.tsdf, vol.weight, vol.origin, vol.voxel, 1.0, capacity=0)
        total = count_only()[1]
        buf = torch.empty((total, 3, 3), dtype=torch.float32, device=eng.device)
        write = lambda: eng.tsdf_triangles(vol.tsdf, vol.weight, vol.origin, vol.voxel, 1.0, capacity=total, out=buf)
        ms_cnt, win_cnt = window(count_only, a.warmup, a.min_ms, a.rounds)
        ms_wr, win_wr = window(write, a.warmup, a.min_ms, a.rounds)
        n_cells = (vol.nx - 1) * (vol.ny - 1) * (vol.nz - 1)
        # torch baselines on copies
        tt, tw = torch.ones_like(vol.tsdf), torch.zeros_like(vol.weight)
        porg = vol.origin
        ms_tint, _ = window(lambda: torch_integrate(tt, tw, porg, vol.voxel, vol.trunc, vol.max_weight, rng, poses, MAX_RANGE), 1,
                            a.min_ms, 3)
        del tt, tw
        ms_tcnt, _ = window(lambda: torch_count(vol.tsdf, vol.weight, 1.0), 1, a.min_ms, 3)
        t_total = torch_count(vol.tsdf, vol.weight, 1.0)[0]
        sec = ms_int * 1e-3
        rec = {
            "voxel": vol.voxel, "trunc": vol.trunc, "shape": list(shape), "samples": vol.n_samples,
            "integration": {
                "ms_per_call": round(ms_int, 4), "windows_ms": win_int, "pairs_in_boxes": pairs, "updates_applied": updates,
                "pairs_per_s": pairs / sec, "updates_per_s": updates / sec,
                "hbm_bytes_per_s": (vol.n_samples * SAMPLE_BYTES) / sec, "share_of_hbm_peak": vol.n_samples * SAMPLE_BYTES / sec / HBM_PEAK,
                "share_of_fp32_vector_peak": pairs * PAIR_FLOPS / sec / FP32_PEAK,
                "torch_ms_per_call": round(ms_tint, 3), "speedup_over_torch": ms_tint / ms_int,
                "one_scan": {"ms_per_call": round(ms_one, 4), "pairs_in_box": pairs_one, "pairs_per_s": pairs_one / (ms_one * 1e-3)},
                "one_blind_scan_ms_per_call": round(ms_blind, 4)},
            "extraction": {
                "triangles": total, "cells": n_cells, "count_ms": round(ms_cnt, 4), "count_windows_ms": win_cnt,
                "count_and_write_ms": round(ms_wr, 4), "write_windows_ms": win_wr, "write_ms": round(ms_wr - ms_cnt, 4),
                "count_hbm_bytes_per_s": n_cells * CELL_BYTES_HBM / (ms_cnt * 1e-3),
                "count_share_of_hbm_peak": n_cells * CELL_BYTES_HBM / (ms_cnt * 1e-3) / HBM_PEAK,
                "write_bytes_per_s": (n_cells * CELL_BYTES_HBM + total * TRIANGLE_BYTES) / max((ms_wr - ms_cnt) * 1e-3, 1e-9),
                "torch_count_and_offsets_ms": round(ms_tcnt, 3), "torch_triangles": t_total, "speedup_over_torch_count": ms_tcnt / ms_cnt}}
        out["volumes"].append(rec)
        if fused_mesh is None:
            fused_mesh = vol.mesh()
        del vol, buf
        torch.cuda.empty_cache()
    # from_mesh on the fused mesh beside the source mesh
    side = int(np.ceil(np.sqrt(a.map_poses)))
    gp = grid_poses((40.0, 40.0 + 4.0 * side), (40.0, 40.0 + 4.0 * side), 4.0, z=0.0)[:a.map_poses]
    gp[:, 2, 3] = ground(gp[:, 0, 3], gp[:, 1, 3]) + SENSOR_Z
    out["from_mesh"] = {"poses": int(len(gp))}
    for name, mesh in (("source", make_mesh(a.grid)), ("fused", fused_mesh)):      # a fresh source object: its hierarchy is not built yet
        t0 = time.perf_counter()
        mesh.bvh
        build_s = time.perf_counter() - t0
        wall = []
        for _ in range(3):
            infer.feature_volumes = FeatureVolumeCache(eng, min_capacity=a.map_poses)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mp = OverlapMap.from_mesh(infer, mesh, gp, resolution=4.0, **sensor)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        out["from_mesh"][name] = {"triangles": mesh.n_triangles, "bvh_build_host_s": round(build_s, 4), "kept": int(len(mp.kept)),
                                  "wall_s_runs": [round(v, 4) for v in wall], "wall_s": round(float(np.median(wall[1:])), 4)}
    print(json.dumps(out, indent=1))
    infer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
