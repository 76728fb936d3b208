"""Raw scans -> the sensor poses the mapping tools take: LiDAR odometry on the GPU (`overlapnet_amd.odometry`).

    python tools/odometry.py --config network.json --scans sequences/07/velodyne --out poses.txt [--mesh site.ply] [--voxel 0.2] \\
        [--frame-to-frame-only] [--window 120 [--keep [--save-volume map.npz]]] \\
        [--deskew --times DIR | --deskew --start-azimuth DEG --clockwise] [--deskew-passes 2]

Every scan is registered onto its predecessor (one launch per chunk of pairs); that trajectory sizes a TSDF volume, and the drive is
then tracked against the volume it builds: each scan is registered onto a ray-cast view of the model at its predicted pose and fused.
--frame-to-frame-only stops after the first pass.  --window M skips the first pass: the volume is a window M metres wide that follows the
sensor, and what leaves it is meshed on the way.  --keep keeps what leaves in a brick store instead and brings it
back when the drive returns; --save-volume writes window and store as one .npz that `tools/build_mesh.py
--load-volume` meshes.  The poses file holds one KITTI pose line per scan (12 numbers, sensor to world in the
sensor frame, the first pose the identity): the file `tools/build_mesh.py --poses` reads without --calib.  --mesh also writes the tracked
volume's zero level set.  The config is the `network.yml` dict `Infer` takes; its `model.inputShape` is the range image the scans are
projected into.  --deskew takes the scans as RAW sweeps and undoes the sensor's motion within each while tracking (DESIGN.md section
37); each pose is then the sensor's at fraction --t-ref of its sweep, and `tools/build_mesh.py --deskew` fuses the same scans at them.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from tools.localize import load_config
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--scans", required=True, help="folder of .bin scans (sorted by name = frame order)")
    ap.add_argument("--out", required=True, help="the poses, one KITTI line per scan")
    ap.add_argument("--mesh", default=None, help="also write the tracked volume's mesh, binary PLY")
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance in metres (default: 4 voxels)")
    ap.add_argument("--window", type=float, default=None, metavar="M", help="track in a volume M metres wide (--below + --above metres "
                    "high) that follows the sensor: no first pass, no limit on the drive's extent; --mesh writes the streamed mesh")
    ap.add_argument("--keep", action="store_true", help="with --window: keep what leaves the window in a brick store and bring it back "
                    "when the drive returns")
    ap.add_argument("--save-volume", default=None, metavar="FILE.npz", help="with --keep: write window and store as one file")
    ap.add_argument("--frame-to-frame-only", action="store_true")
    ap.add_argument("--min-fitness", type=float, default=None, help="a registration below it counts as failed (default: none)")
    ap.add_argument("--below", type=float, default=5.0, help="metres of volume below the lowest sensor position")
    ap.add_argument("--above", type=float, default=15.0, help="metres of volume above the highest sensor position")
    ap.add_argument("--chunk", type=int, default=64, help="pairs registered per launch in the first pass")
    ap.add_argument("--fov-up", type=float, default=3.0)
    ap.add_argument("--fov-down", type=float, default=-25.0)
    ap.add_argument("--max-range", type=float, default=50.0)
    ap.add_argument("--min-range", type=float, default=0.5, help="where a ray of the model's view starts")
    from overlapnet_amd import deskew as motion
    motion.add_arguments(ap)
    ap.add_argument("--deskew-passes", type=int, default=1, choices=(1, 2), help="2: deskew each scan again, by the step its "
                    "registration found, before it is fused")
    a = ap.parse_args(argv)
    deskew = motion.config_from_args(ap, a)
    if a.keep and a.window is None:
        ap.error("--keep belongs to --window")
    if a.save_volume is not None and not a.keep:
        ap.error("--save-volume belongs to --keep")
    if a.keep and a.frame_to_frame_only:
        ap.error("--keep belongs to the tracker: drop --frame-to-frame-only")
    if deskew is not None and a.frame_to_frame_only:
        ap.error("--deskew belongs to the tracker: drop --frame-to-frame-only")

    cfg = load_config(a.config)
    h, w = (int(v) for v in cfg["model"]["inputShape"][:2])
    paths = sorted(os.path.join(a.scans, f) for f in os.listdir(a.scans) if f.endswith(".bin"))
    if not paths:
        raise SystemExit("no .bin scans in %s" % a.scans)
    if a.chunk < 1:
        raise SystemExit("--chunk must be >= 1")
    if a.mesh and a.frame_to_frame_only:
        raise SystemExit("--mesh needs the tracked volume: drop --frame-to-frame-only")
    scans = [np.fromfile(p, dtype=np.float32).reshape((-1, 4)) for p in paths]
    offsets = np.zeros(len(scans) + 1, np.int64)
    offsets[1:] = np.cumsum([c.shape[0] for c in scans])
    points = np.concatenate(scans)
    times = None
    if a.times is not None:
        try:
            times = motion.read_times(a.times, paths, [c.shape[0] for c in scans])
        except ValueError as e:
            raise SystemExit("odometry: %s" % e)

    from overlapnet_amd import odometry
    from overlapnet_amd.engine import OvnEngine
    sensor = dict(proj_h=h, proj_w=w, fov_up=a.fov_up, fov_down=a.fov_down, max_range=a.max_range)
    t0 = time.time()
    eng = OvnEngine()                            # the projection takes its image shape per call
    try:
        line = {"out": a.out, "scans": len(paths)}
        if a.frame_to_frame_only:
            poses, regs = odometry.frame_to_frame(eng, points, offsets, chunk=a.chunk, **sensor)
            line.update(mode="frame_to_frame", failed_pairs=int(sum(r.status != 0 for r in regs)))
        else:
            try:
                poses, results, vol = odometry.estimate_poses(eng, points, offsets, voxel=a.voxel, trunc=a.trunc, min_range=a.min_range,
                                                              below=a.below, above=a.above, chunk=a.chunk, min_fitness=a.min_fitness,
                                                              window=a.window, keep=a.keep, deskew=deskew, times=times,
                                                              deskew_passes=a.deskew_passes, **sensor)
            except ValueError as e:
                raise SystemExit("odometry: %s" % e)
            line.update(mode="frame_to_model", volume=[vol.nx, vol.ny, vol.nz], voxel=vol.voxel,
                        sources={s: int(sum(r.source == s for r in results)) for s in ("first", "model", "frame", "prediction")})
            if deskew is not None:
                line.update(deskew=dict(deskew, passes=a.deskew_passes, times=a.times))
            if a.window is not None:
                line.update(window_m=a.window, window_shifts=vol.n_shifts)
            if a.keep:
                line.update(stored_bricks=len(vol.store), stored_bytes=vol.store.bytes)
                if a.save_volume is not None:
                    line.update(saved_volume=a.save_volume, saved_bricks=vol.store.save(a.save_volume, window=vol))
            if a.mesh:
                mesh = vol.mesh()
                mesh.to_ply(a.mesh)
                line.update(mesh=a.mesh, triangles=mesh.n_triangles)
        odometry.write_poses(a.out, poses)
        line["seconds"] = round(time.time() - t0, 3)
        print(json.dumps(line))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
