"""Raw scans + sensor poses -> the triangle mesh `tools/localize.py --mesh` takes: the scans' range images fused into a truncated signed
distance volume on the GPU and its zero level set extracted (`overlapnet_amd.tsdf`).

    python tools/build_mesh.py --config network.json --scans sequences/07/velodyne --poses poses/07.txt --calib sequences/07/calib.txt \\
        --voxel 0.2 --out site.ply [--bounds X0 Y0 Z0 X1 Y1 Z1] [--every N] [--deskew --times DIR | --deskew --start-azimuth DEG --clockwise]
    python tools/build_mesh.py --load-volume map.npz --out site.ply          # mesh what `tools/odometry.py --keep --save-volume` wrote

The config is the `network.yml` dict `Infer` takes (JSON, or YAML when PyYAML is installed): its `model.inputShape` is the range image
the scans are projected into.  The poses file holds one pose per line (12 numbers, a 3 x 4 matrix) or is an npz of (n,4,4) matrices,
read as `tools/build_training_set.py` reads it.  With --calib they are camera poses and are moved into the LiDAR frame of the first
scan with the calibration's `Tr:` line; without it they are taken as sensor-to-world poses as they stand.  Without --bounds the
volume is the poses' bounding box grown by --max-range (and by --below / --above in z); a volume over 2^31 - 1 samples is refused with
the voxel size that would fit.  --deskew takes the scans as RAW sweeps: each is moved into the sensor frame of fraction --t-ref of its
sweep under the twist of the step that led to its pose (of ALL the poses, whatever --every says) before it is
projected, and the poses are taken as the sensor's at that fraction, which is what `tools/odometry.py --deskew` writes.  --load-volume
meshes a saved brick store without scans: --config, --scans and --poses are then not needed.  Prints one JSON
line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def default_bounds(poses: np.ndarray, max_range: float, below: float, above: float):
    """(lo, hi): the sensor positions' bounding box grown by max_range in x and y, by `below` / `above` metres in z
    (`overlapnet_amd.odometry.bounds_from_poses`, which the odometry sizes its own volume with)."""
    from overlapnet_amd.odometry import bounds_from_poses
    return bounds_from_poses(poses, max_range, below, above)


def mesh_saved_volume(a) -> None:
    """--load-volume: the mesh of a saved brick store, every cell once."""
    from overlapnet_amd.engine import OvnEngine
    from overlapnet_amd.tsdf_store import TsdfBrickStore, mesh_from_store
    t0 = time.time()
    eng = OvnEngine()
    try:
        store = TsdfBrickStore.load(eng, a.load_volume)
        mesh = mesh_from_store(store, min_weight=a.min_weight)
        mesh.to_ply(a.out)
        print(json.dumps({"out": a.out, "loaded_volume": a.load_volume, "bricks": len(store), "voxel": store.meta["voxel"],
                          "trunc": store.meta["trunc"], "triangles": mesh.n_triangles, "seconds": round(time.time() - t0, 3)}))
    finally:
        eng.close()


def main(argv=None):
    from tools.build_training_set import lidar_poses, read_calib, read_poses
    from tools.localize import load_config
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default=None)
    ap.add_argument("--scans", default=None, help="folder of .bin scans (sorted by name = frame order)")
    ap.add_argument("--poses", default=None)
    ap.add_argument("--load-volume", default=None, metavar="FILE.npz", help="mesh the brick store `tools/odometry.py --keep "
                    "--save-volume` wrote, without scans")
    ap.add_argument("--calib", default=None, help="KITTI calib.txt: the poses are camera poses")
    ap.add_argument("--out", required=True, help="the mesh, binary PLY")
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance in metres (default: 4 voxels)")
    ap.add_argument("--max-weight", type=float, default=64.0)
    ap.add_argument("--min-weight", type=float, default=1.0, help="a cell needs all eight corners seen this often")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--below", type=float, default=5.0, help="without --bounds: metres below the lowest sensor position")
    ap.add_argument("--above", type=float, default=15.0, help="without --bounds: metres above the highest sensor position")
    ap.add_argument("--every", type=int, default=1, help="fuse every N-th scan")
    ap.add_argument("--chunk", type=int, default=64, help="scans projected and fused per pass")
    ap.add_argument("--fov-up", type=float, default=3.0)
    ap.add_argument("--fov-down", type=float, default=-25.0)
    ap.add_argument("--max-range", type=float, default=50.0)
    from overlapnet_amd import deskew as motion
    motion.add_arguments(ap)
    a = ap.parse_args(argv)
    deskew = motion.config_from_args(ap, a)
    if a.load_volume is not None:
        if a.config or a.scans or a.poses or deskew is not None:
            ap.error("--load-volume meshes a saved volume: it takes no --config, --scans, --poses or --deskew")
        return mesh_saved_volume(a)
    missing = [n for n in ("config", "scans", "poses") if getattr(a, n) is None]
    if missing:
        ap.error("the following arguments are required: %s" % ", ".join("--" + n for n in missing))

    cfg = load_config(a.config)
    h, w = (int(v) for v in cfg["model"]["inputShape"][:2])
    paths = sorted(os.path.join(a.scans, f) for f in os.listdir(a.scans) if f.endswith(".bin"))
    poses = read_poses(a.poses)
    if a.calib:
        poses = lidar_poses(poses, read_calib(a.calib))
    if len(paths) != len(poses):
        raise SystemExit("%d scans in %s but %d poses in %s" % (len(paths), a.scans, len(poses), a.poses))
    if a.every < 1 or a.chunk < 1:
        raise SystemExit("--every and --chunk must be >= 1")
    twists = motion.twists_from_poses(poses)[::a.every] if deskew is not None else None
    paths, poses = paths[::a.every], poses[::a.every]
    if not paths:
        raise SystemExit("no .bin scans in %s" % a.scans)
    lo, hi = (np.asarray(a.bounds[:3]), np.asarray(a.bounds[3:])) if a.bounds else default_bounds(poses, a.max_range, a.below, a.above)

    from overlapnet_amd import tsdf
    from overlapnet_amd.engine import OvnEngine
    try:
        tsdf.volume_shape(lo, hi, a.voxel)            # refuse an oversized volume before a GPU is touched
    except ValueError as e:
        raise SystemExit("build_mesh: %s" % e)
    t0 = time.time()
    eng = OvnEngine()                            # the projection takes its image shape per call
    try:
        vol = tsdf.TsdfVolume(eng, lo, hi, a.voxel, trunc=a.trunc, max_weight=a.max_weight)
        for s in range(0, len(paths), a.chunk):
            scans = [np.fromfile(p, dtype=np.float32).reshape((-1, 4)) for p in paths[s:s + a.chunk]]
            offsets = np.zeros(len(scans) + 1, np.int64)
            offsets[1:] = np.cumsum([c.shape[0] for c in scans])
            extra = {}
            if deskew is not None:
                extra = dict(deskew=deskew, twists=twists[s:s + a.chunk])
                if a.times is not None:
                    try:
                        extra["times"] = motion.read_times(a.times, paths[s:s + a.chunk], [c.shape[0] for c in scans])
                    except ValueError as e:
                        raise SystemExit("build_mesh: %s" % e)
            vol.integrate_scans(np.concatenate(scans), offsets, poses[s:s + a.chunk], proj_h=h, proj_w=w, fov_up=a.fov_up,
                                fov_down=a.fov_down, max_range=a.max_range, chunk=a.chunk, **extra)
        mesh = vol.mesh(a.min_weight)
        mesh.to_ply(a.out)
        print(json.dumps({"out": a.out, "scans": len(paths), "volume": [vol.nx, vol.ny, vol.nz], "voxel": vol.voxel, "trunc": vol.trunc,
                          "lo": [float(v) for v in lo], "triangles": mesh.n_triangles, "seconds": round(time.time() - t0, 3)}))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
