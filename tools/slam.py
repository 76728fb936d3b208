"""Raw scans -> loop-closed poses: odometry, OverlapNet candidates, ICP verification, pose-graph optimization, all on the GPU
(`overlapnet_amd.pose_graph`).

    python tools/slam.py --config network.json --scans sequences/07/velodyne --out poses.txt [--poses odometry.txt] [--mesh site.ply] \\
        --overlap-thres 0.3 --min-fitness 0.5 --max-rms none --odom-sigma 0.05 0.01 --loop-sigma 0.1 0.02 --huber 1.5 \\
        [--deskew --times DIR | --deskew --start-azimuth DEG --clockwise]

  1  poses: `odometry.estimate_poses` on the scans, or the KITTI pose lines of --poses (12 numbers per line, sensor frame)
  2  candidates: `Infer` on the raw scans (`scan_folder` = --scans, frames 000000.bin ...): `cache_frames`, then per frame
     `infer_top_k_batch` against the frames at least --min-gap frames earlier
  3  verification: `Infer.verify_top_k` for every frame that has a candidate: one ICP launch per frame
  4  graph: the odometry steps and the accepted loop closures, `PoseGraph.optimize`
  5  --out: the optimized poses (`odometry.write_poses`); --mesh: the scans re-fused at them (`TsdfVolume`); --covariances: the
     optimized graph's marginal pose covariances (`PoseGraph.marginals`, `lcd.write_covariances`)
--deskew takes the scans as RAW sweeps: step 1 tracks with motion compensation, and --mesh deskews every scan
by the optimized poses' own steps before it is fused.  Steps 2 and 3 see the scans as they are on disk.
--gate-sigma N narrows step 2 to the frames inside the N-sigma ellipse of dead reckoning's covariance; it has no default value.

--overlap-thres, --min-fitness, --max-rms, --odom-sigma, --loop-sigma and --huber have no defaults: no acceptance threshold or noise
level has been measured on real loop closures, so each is given or is explicitly `none` (thresholds and --huber; with both --min-fitness
and --max-rms `none`, every registration that finished becomes an edge).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def number_or_none(text):
    return None if text.strip().lower() == "none" else float(text)


def read_pose_lines(path):
    """(n,4,4) float64 from KITTI pose lines (12 numbers per line)."""
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    if rows.shape[1] != 12:
        raise ValueError("%s: expected 12 numbers per line, got %d" % (path, rows.shape[1]))
    poses = np.tile(np.eye(4), (rows.shape[0], 1, 1))
    poses[:, :3, :] = rows.reshape(-1, 3, 4)
    return poses


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--scans", required=True, help="folder of .bin scans named 000000.bin, 000001.bin, ...")
    ap.add_argument("--out", required=True, help="the optimized poses, one KITTI line per scan")
    ap.add_argument("--poses", default=None, help="take the odometry from this file instead of tracking the scans")
    ap.add_argument("--mesh", default=None, help="also re-fuse the scans at the optimized poses and write the mesh, binary PLY")
    ap.add_argument("--min-gap", type=int, default=50, help="a loop closure joins frames at least this many frames apart")
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--overlap-thres", type=number_or_none, required=True)
    ap.add_argument("--min-fitness", type=number_or_none, required=True)
    ap.add_argument("--max-rms", type=number_or_none, required=True)
    ap.add_argument("--odom-sigma", type=float, nargs=2, required=True, metavar=("METRES", "RADIANS"))
    ap.add_argument("--loop-sigma", type=float, nargs=2, required=True, metavar=("METRES", "RADIANS"))
    ap.add_argument("--huber", type=number_or_none, required=True)
    ap.add_argument("--max-iterations", type=int, default=30)
    ap.add_argument("--preconditioner", default="auto", choices=("auto", "auto+loops", "jacobi", "chain", "loops"))
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--window", type=float, default=None, metavar="M", help="track (and mesh) in a TSDF window M metres wide that follows "
                    "the sensor instead of a volume over the whole drive")
    ap.add_argument("--keep", action="store_true", help="with --window: keep what leaves the window in a brick store, for tracking and for "
                    "the re-fusion at the optimized poses, so that a revisited street is one surface (DESIGN.md section 38)")
    ap.add_argument("--fov-up", type=float, default=3.0)
    ap.add_argument("--fov-down", type=float, default=-25.0)
    ap.add_argument("--max-range", type=float, default=50.0)
    ap.add_argument("--batch", type=int, default=64, help="frames per `infer_top_k_batch` call")
    ap.add_argument("--covariances", default=None, help="also write the optimized graph's marginal pose covariances (position frame), "
                    "one line of 36 numbers per scan: the covariance file of the reference's loop-closure demo")
    ap.add_argument("--gate-sigma", type=float, default=None, help="for frame k take only candidates inside the N-sigma x, y ellipse of "
                    "the odometry-only graph's marginal covariance at k (with --min-gap); not given: every earlier frame")
    from overlapnet_amd import deskew as motion
    motion.add_arguments(ap)
    a = ap.parse_args(argv)
    a.deskew_config = motion.config_from_args(ap, a)
    if a.keep and a.window is None:
        ap.error("--keep belongs to --window")
    if a.min_gap < 1 or a.top_k < 1 or a.batch < 1:
        ap.error("--min-gap, --top-k and --batch must be >= 1")
    if a.gate_sigma is not None and not a.gate_sigma > 0.0:
        ap.error("--gate-sigma must be > 0")
    return a


def main(argv=None):
    a = parse(argv)
    from tools.localize import load_config
    cfg = dict(load_config(a.config))
    cfg["scan_folder"] = a.scans
    h, w = (int(v) for v in cfg["model"]["inputShape"][:2])
    names = sorted(f for f in os.listdir(a.scans) if f.endswith(".bin"))
    if names != ["%06d.bin" % i for i in range(len(names))] or not names:
        raise SystemExit("%s must hold the scans 000000.bin .. without a gap (Infer addresses frames by number)" % a.scans)
    n = len(names)
    scans = [np.fromfile(os.path.join(a.scans, f), dtype=np.float32).reshape((-1, 4)) for f in names]
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([c.shape[0] for c in scans])
    points = np.concatenate(scans)

    from overlapnet_amd import deskew as motion, lcd, odometry, pose_graph, tsdf
    times = None
    if a.times is not None:
        try:
            times = motion.read_times(a.times, [os.path.join(a.scans, f) for f in names], [c.shape[0] for c in scans])
        except ValueError as e:
            raise SystemExit("slam: %s" % e)
    from overlapnet_amd.infer import Infer
    t0 = time.time()
    infer = Infer(cfg)
    eng = infer.engine
    sensor = dict(proj_h=h, proj_w=w, fov_up=a.fov_up, fov_down=a.fov_down, max_range=a.max_range)
    if a.poses:
        poses = read_pose_lines(a.poses)
        if poses.shape[0] != n:
            raise SystemExit("%s holds %d poses for %d scans" % (a.poses, poses.shape[0], n))
    else:
        poses, _, _ = odometry.estimate_poses(eng, points, offsets, voxel=a.voxel, window=a.window, keep=a.keep, deskew=a.deskew_config,
                                              times=times, **sensor)
    line = {"out": a.out, "scans": n, "odometry_seconds": round(time.time() - t0, 3)}

    infer.cache_frames(n)
    queries = list(range(a.min_gap, n))
    references = {c: np.arange(0, c - a.min_gap + 1) for c in queries}
    if a.gate_sigma is not None:      # the search space of the reference's demo: the ellipse of dead reckoning's covariance at the frame
        dead = pose_graph.PoseGraph(eng, poses)
        dead.add_odometry(poses, pose_graph.information_from_sigmas(*a.odom_sigma))
        ellipses = lcd.ellipses_from_covariances(dead.marginals(frame="position"), a.gate_sigma)
        xy = poses[:, :2, 3]
        length = lcd.travelled_distances(xy)
        references = {c: lcd.gate_candidates(c, xy, length, ellipses[c], inactive_time_thres=a.min_gap - 1,
                                             inactive_dist_thres=-np.inf) for c in queries}
        queries = [c for c in queries if len(references[c])]
        line["frames_with_gated_candidates"] = len(queries)
    with_candidates = []
    for s in range(0, len(queries), a.batch):
        cur = queries[s:s + a.batch]
        found = infer.infer_top_k_batch(cur, [references[c] for c in cur], k=a.top_k, overlap_thres=a.overlap_thres)
        with_candidates += [c for c, f in zip(cur, found) if f]
    graph = pose_graph.PoseGraph(eng, poses)
    graph.add_odometry(poses, pose_graph.information_from_sigmas(*a.odom_sigma))
    loop_info = pose_graph.information_from_sigmas(*a.loop_sigma)
    thresholds = a.min_fitness is not None or a.max_rms is not None
    verified = 0
    for c in with_candidates:
        checked = infer.verify_top_k(c, references[c], k=a.top_k, overlap_thres=a.overlap_thres,
                                     min_fitness=a.min_fitness, max_rms=a.max_rms)
        verified += len(checked)
        graph.add_loop_closures(c, checked, loop_info, only_accepted=thresholds)
    loops = len(graph.edges) - (n - 1)
    line.update(frames_with_candidates=len(with_candidates), candidates_verified=verified, loop_edges=loops)
    res = graph.optimize(max_iterations=a.max_iterations, huber=a.huber, preconditioner=a.preconditioner)
    odometry.write_poses(a.out, res.poses)
    moved = np.linalg.norm(res.poses[:, :3, 3] - poses[:, :3, 3], axis=1)
    line.update(preconditioner=graph.choose_preconditioner(a.preconditioner), outer_iterations=res.outer_iterations,
                cg_iterations=res.cg_iterations, converged=bool(res.converged), cost_initial=res.cost_initial, cost_final=res.cost_final,
                loop_edges_turned_down=int((res.weights[n - 1:] < 1.0).sum()), largest_correction_m=float(moved.max()))
    if a.covariances:
        lcd.write_covariances(a.covariances, graph.marginals(frame="position", huber=a.huber))
        line["covariances"] = a.covariances
    if a.mesh:
        fuse = lambda lo, hi: {}
        if a.deskew_config is not None:
            twists = motion.twists_from_poses(res.poses)
            fuse = lambda lo, hi: dict(deskew=a.deskew_config, twists=twists[lo:hi],
                                       **({} if times is None else dict(times=times[int(offsets[lo]):int(offsets[hi])])))
        if a.window is not None:      # the window follows the optimized poses; what leaves it is meshed on the way
            vol = tsdf.RollingTsdfVolume(eng, (a.window, a.window, 20.0), a.voxel, store=True if a.keep else None)
            for s in range(n):
                vol.follow(res.poses[s, :3, 3])
                vol.integrate_scans(points[int(offsets[s]):int(offsets[s + 1])], [0, int(offsets[s + 1] - offsets[s])], res.poses[s:s + 1],
                                    **sensor, **fuse(s, s + 1))
        else:
            lo, hi = odometry.bounds_from_poses(res.poses, a.max_range)
            vol = tsdf.TsdfVolume(eng, lo, hi, a.voxel)
            vol.integrate_scans(points, offsets, res.poses, **sensor, **fuse(0, n))
        mesh = vol.mesh()
        mesh.to_ply(a.mesh)
        line.update(mesh=a.mesh, triangles=mesh.n_triangles)
    line["seconds"] = round(time.time() - t0, 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
