"""Throughput of `ovn_render_scans` (csrc/render_mesh.hip) and of `OverlapMap.from_mesh` on a synthetic mesh made here from a seed.

The mesh: a 200 m x 200 m height field (a few sine waves, 3 m of relief) with square "buildings" raised 8 m, n x n quads of two
triangles each; n = 71, 224, 707 gives about 10^4, 10^5 and 10^6 triangles.  The sensor: 64 x 900, the reference's field of view,
max_range 50 m, 1.7 m above the ground at random positions and headings.

Per mesh size: the host build time of the hierarchy (NumPy, `mesh.build_bvh`), and rays/s of the hierarchy route -- `--poses` scans per
call, `--warmup` untimed calls, then calls between two HIP events until `--min-ms` of device time have passed, the median of
`--rounds` such windows.  At the smallest size the same for the exhaustive route (fewer poses per call).  What a ray fetches is
COUNTED, not measured: `count_ray_work` walks the same tree in the same order on the host for a sample of rays and counts the child
pairs (64 B of boxes each) and triangles (4 B of order, 12 B of indices, 36 B of vertices) a ray touches; bytes/ray times rays/s over
the HBM peak, and the floating-point operations of those slab tests and intersections over the fp32 vector peak, say how far the
kernel is from either limit.  Then `OverlapMap.from_mesh` on `--map-poses` grid poses with test weights: the whole call by the host
clock (it ends in a synchronise), and its three stages on one chunk by events -- the ray kernel alone (range and vertex images), the
normals + stacking pass (the call that also asks for the stacked input, minus the former), and the leg.  ONE JSON object on stdout.

    python tools/bench_render.py > profiles/render.json"""
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

H, W, FOV_UP, FOV_DOWN, MAX_RANGE, SENSOR_Z = 64, 900, 3.0, -25.0, 50.0, 1.7
EXTENT = 200.0
HBM_PEAK, FP32_PEAK = 8.0e12, 157.3e12          # bytes/s and FLOP/s (spec)
PAIR_BYTES, TRI_BYTES = 64, 4 + 12 + 36
PAIR_FLOPS, TRI_FLOPS = 2 * 30, 62              # two slab tests (per axis 2 sub, 4 mul, 4 compare-selects); one Moeller-Trumbore


def ground(x, y):
    z = 1.5 * np.sin(x / 17.0) + 1.0 * np.cos(y / 11.0) + 0.5 * np.sin((x + y) / 5.0)
    cx, cy = np.floor(x / 25.0), np.floor(y / 25.0)
    inside = (np.abs(x - (cx + 0.5) * 25.0) < 5.0) & (np.abs(y - (cy + 0.5) * 25.0) < 5.0) & ((cx + cy) % 2 == 0)
    return np.where(inside, z + 8.0, z)


def make_mesh(n):
    from overlapnet_amd.mesh import TriangleMesh
    a = np.linspace(0.0, EXTENT, n + 1)
    x, y = np.meshgrid(a, a, indexing="xy")
    v = np.stack([x, y, ground(x, y)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    p00, p10, p01, p11 = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    t = np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)]).astype(np.int32)
    return TriangleMesh(v, t)


def make_poses(n, seed):
    g = np.random.default_rng(seed)
    out = np.zeros((n, 4, 4))
    k = 0
    while k < n:
        x, y, yaw = g.uniform(20.0, EXTENT - 20.0), g.uniform(20.0, EXTENT - 20.0), g.uniform(-np.pi, np.pi)
        z = float(ground(np.float64(x), np.float64(y)))
        if z > 5.0:          # on a roof
            continue
        c, s = np.cos(yaw), np.sin(yaw)
        out[k] = [[c, -s, 0, x], [s, c, 0, y], [0, 0, 1, z + SENSOR_Z], [0, 0, 0, 1]]
        k += 1
    return out


def window(fn, warmup, min_ms, rounds):
    """Median over `rounds` windows of the milliseconds per call of fn, each window at least min_ms of device time."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        calls, ms = 0, 0.0
        a.record()
        while True:
            fn()
            calls += 1
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= min_ms:
                break
        per_call.append(ms / calls)
    return float(np.median(per_call)), [round(v, 4) for v in per_call]


def count_ray_work(mesh, poses, n_rays, seed):
    """Mean child pairs and triangles a ray touches: the traversal of render_bvh_kernel (near child first, pruned against the best t,
    deferred siblings re-checked on pop) walked on the host in float64 for a random sample of rays."""
    from overlapnet_amd.mesh import direction_tables, LEAF_TRIANGLES
    nodes, order, nl = mesh.bvh
    lo, hi = nodes[:, 0:3].astype(np.float64), nodes[:, 4:7].astype(np.float64)
    v, tri = mesh.vertices.astype(np.float64), mesh.triangles
    ca, sa, cp, sp = (t.astype(np.float64) for t in direction_tables(H, W, FOV_UP, FOV_DOWN))
    g = np.random.default_rng(seed)
    pairs = tris = hits = 0

    def slab(i, o, inv, limit):
        if lo[i, 0] > hi[i, 0]:
            return -1.0
        with np.errstate(invalid="ignore", over="ignore"):
            t0, t1 = (lo[i] - o) * inv, (hi[i] - o) * inv
        tn = max(0.0, float(np.nanmax(np.minimum(t0, t1), initial=0.0)))
        tf = min(limit, float(np.nanmin(np.maximum(t0, t1), initial=limit)))
        return tn if tn <= tf else -1.0

    for _ in range(n_rays):
        P = poses[g.integers(len(poses))]
        py, px = g.integers(H), g.integers(W)
        d = P[:3, :3] @ np.array([cp[py] * ca[px], cp[py] * sa[px], sp[py]])
        o = P[:3, 3]
        with np.errstate(divide="ignore"):
            inv = 1.0 / d
        best = np.inf
        if slab(1, o, inv, MAX_RANGE) < 0:
            continue
        stack, node = [], 1
        while True:
            if node < nl:
                lim = min(best, MAX_RANGE)
                pairs += 1
                t0, t1 = slab(2 * node, o, inv, lim), slab(2 * node + 1, o, inv, lim)
                if t0 >= 0 and t1 >= 0:
                    first0 = t0 <= t1
                    stack.append((2 * node + 1, t1) if first0 else (2 * node, t0))
                    node = 2 * node if first0 else 2 * node + 1
                    continue
                if t0 >= 0 or t1 >= 0:
                    node = 2 * node if t0 >= 0 else 2 * node + 1
                    continue
            else:
                f = (node - nl) * LEAF_TRIANGLES
                for k in order[f:f + LEAF_TRIANGLES]:
                    tris += 1
                    v0, v1, v2 = v[tri[k]]
                    e1, e2 = v1 - v0, v2 - v0
                    p = np.cross(d, e2)
                    det = e1 @ p
                    if det == 0:
                        continue
                    s = o - v0
                    u = (s @ p) / det
                    q = np.cross(s, e1)
                    w = (d @ q) / det
                    t = (e2 @ q) / det
                    if u >= 0 and w >= 0 and u + w <= 1 and 0 < t < MAX_RANGE and t < best:
                        best = t
            node = None
            while stack:
                cand, tn = stack.pop()
                if not tn > best:
                    node = cand
                    break
            if node is None:
                break
        hits += best < np.inf
    return pairs / n_rays, tris / n_rays, hits / n_rays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, nargs="+", default=[71, 224, 707], help="quads per side of the height field")
    ap.add_argument("--poses", type=int, default=64)
    ap.add_argument("--exhaustive-poses", type=int, default=2)
    ap.add_argument("--map-poses", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--count-rays", type=int, default=512)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_render needs the MI355X: there is no CPU path and no figure to report without it")
    from tools import synthetic as S
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.localization import OverlapMap, grid_poses, render_chunk
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[H, W]), "infer_seqs": "07", "data_root_folder": tempfile.mkdtemp(),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    infer = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    eng = infer.engine
    sensor = dict(fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE)
    out = {"sensor": dict(H=H, W=W, **sensor), "device": torch.cuda.get_device_name(0), "peaks": {"hbm_bytes_per_s": HBM_PEAK,
           "fp32_vector_flop_per_s": FP32_PEAK}, "meshes": []}
    poses = make_poses(a.poses, 1)
    rays = a.poses * H * W
    meshes = []
    for n in a.grid:
        mesh = make_mesh(n)
        t0 = time.perf_counter()
        nodes, order, nl = mesh.bvh
        build_s = time.perf_counter() - t0
        meshes.append(mesh)
        ms, windows = window(lambda: eng.render_scans(mesh, poses, H, W, want=("range", "tri_id"), **sensor), a.warmup, a.min_ms, a.rounds)
        r = eng.render_scans(mesh, poses, H, W, want=("range",), **sensor)["range"]
        pairs, tris, hit = count_ray_work(mesh, poses, a.count_rays, 2)
        rate = rays / (ms * 1e-3)
        bytes_ray, flops_ray = pairs * PAIR_BYTES + tris * TRI_BYTES, pairs * PAIR_FLOPS + tris * TRI_FLOPS
        out["meshes"].append({
            "grid": n, "triangles": mesh.n_triangles, "leaves": nl, "bvh_build_host_s": round(build_s, 4),
            "bvh_bytes": int(nodes.nbytes + order.nbytes), "poses_per_call": a.poses, "ms_per_call": round(ms, 4), "windows_ms": windows,
            "rays_per_s": rate, "hit_fraction": float((r > 0).float().mean().item()),
            "counted_on_host": {"rays_sampled": a.count_rays, "child_pairs_per_ray": round(pairs, 2), "triangles_per_ray": round(tris, 2),
                                "hit_fraction": round(hit, 3), "bytes_requested_per_ray": round(bytes_ray, 1),
                                "flop_per_ray": round(flops_ray, 1)},
            "bytes_requested_per_s": rate * bytes_ray, "share_of_hbm_peak_if_nothing_hit_a_cache": rate * bytes_ray / HBM_PEAK,
            "share_of_fp32_vector_peak": rate * flops_ray / FP32_PEAK})
    small = meshes[0]
    ep = poses[:a.exhaustive_poses]
    ms, windows = window(lambda: eng.render_scans(small, ep, H, W, want=("range", "tri_id"), exhaustive=True, **sensor), 1, a.min_ms,
                         max(1, a.rounds // 2))
    pair_tests = len(ep) * H * W * small.n_triangles
    out["exhaustive"] = {"triangles": small.n_triangles, "poses_per_call": len(ep), "ms_per_call": round(ms, 3), "windows_ms": windows,
                         "rays_per_s": len(ep) * H * W / (ms * 1e-3), "ray_triangle_tests_per_s": pair_tests / (ms * 1e-3),
                         "share_of_fp32_vector_peak": pair_tests * TRI_FLOPS / (ms * 1e-3) / FP32_PEAK}
    # from_mesh on a grid of poses over the middle mesh
    mesh = meshes[min(1, len(meshes) - 1)]
    side = int(np.ceil(np.sqrt(a.map_poses)))
    gp = grid_poses((40.0, 40.0 + 4.0 * side), (40.0, 40.0 + 4.0 * side), 4.0, z=0.0)[:a.map_poses]
    gp[:, 2, 3] = ground(gp[:, 0, 3], gp[:, 1, 3]) + SENSOR_Z
    from overlapnet_amd.infer import FeatureVolumeCache
    wall = []
    for _ in range(3):
        infer.feature_volumes = FeatureVolumeCache(eng, min_capacity=a.map_poses)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mp = OverlapMap.from_mesh(infer, mesh, gp, resolution=4.0, **sensor)
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    chunk = render_chunk(H, W, 4)
    cp_ = gp[:chunk]
    t_ray, _ = window(lambda: eng.render_scans(mesh, cp_, H, W, want=("range", "vertex"), **sensor), 1, a.min_ms, 3)
    t_all, _ = window(lambda: eng.render_scans(mesh, cp_, H, W, want=("range", "vertex"), stacked_flags=(True, True), **sensor), 1,
                      a.min_ms, 3)
    stk = eng.render_scans(mesh, cp_, H, W, want=(), stacked_flags=(True, True), **sensor)["stacked"]
    t_leg, _ = window(lambda: eng.leg(stk), 1, a.min_ms, 3)
    per = 1.0 / len(cp_)
    out["from_mesh"] = {"triangles": mesh.n_triangles, "poses": int(len(gp)), "kept": int(len(mp.kept)), "chunk": chunk,
                        "wall_s_runs": [round(v, 4) for v in wall], "wall_s": round(float(np.median(wall[1:])), 4),
                        "ms_per_pose": {"ray_kernel": round(t_ray * per, 5), "normals_and_stacking": round((t_all - t_ray) * per, 5),
                                        "leg": round(t_leg * per, 5)}}
    print(json.dumps(out, indent=1))
    infer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
