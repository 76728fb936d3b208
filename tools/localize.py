"""Localize a drive in a saved map with the overlap-based Monte Carlo localization (`overlapnet_amd.localization`).

Build and save a map (keyframe rows `frame x y heading[rad]`, frames named as `Infer` names them):

    python tools/localize.py --config network.json --scans map_scans/ --build keyframes.txt --map map.npz --resolution 1.0

Build the map from a triangle mesh instead (PLY or OBJ): virtual scans rendered on the GPU, one per cell of the grid of --resolution laid
over the mesh's x / y bounding box (`--build grid`) or at the rows `name x y heading` of a file, the sensor --grid-height above z = 0:

    python tools/localize.py --config network.json --mesh site.ply --build grid --map map.npz --resolution 1.0 --grid-height 1.7

Localizing in such a map takes the mesh again (`--mesh site.ply`): its scans are re-rendered, not stored.

Localize (odometry rows `frame dx dy dtheta`: the motion in the robot frame since the previous row, the scan `<scans>/<frame>.bin`):

    python tools/localize.py --config network.json --map map.npz --map-scans map_scans/ --scans drive_scans/ --odom odom.txt \\
        --particles 10000 --sigma 0.1 0.1 0.02

The config is the `network.yml` dict `Infer` takes, as JSON (or YAML when PyYAML is installed); `--scans` / `--map-scans` set its
`scan_folder` (raw .bin scans, projected on the GPU).  One line per step on stdout:
`frame x y heading n_eff frames_scored off_map resampled lost`.  The observation-model defaults are untuned (see the module)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_config(path):
    with open(path) as f:
        if path.endswith((".yml", ".yaml")):
            import yaml
            return yaml.safe_load(f)
        return json.load(f)


def read_rows(path):
    """(names, (n,3) float64) from rows `name a b c`; '#' starts a comment."""
    names, vals = [], []
    with open(path) as f:
        for line in f:
            t = line.split("#")[0].split()
            if not t:
                continue
            if len(t) != 4:
                raise ValueError("%s: expected `frame a b c`, got %r" % (path, line.strip()))
            names.append(t[0])
            vals.append([float(v) for v in t[1:]])
    return names, np.asarray(vals, np.float64).reshape(-1, 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--map", required=True, help="the saved map (.npz): written with --build, read otherwise")
    ap.add_argument("--scans", help="folder of the .bin scans named by --build / --odom")
    ap.add_argument("--map-scans", help="folder of the map's .bin scans when it differs from --scans")
    ap.add_argument("--build", help="keyframe file: build the map, save it and exit")
    ap.add_argument("--mesh", help="triangle mesh (.ply / .obj): --build renders the map's scans from it; needed again to localize in such a map")
    ap.add_argument("--grid-height", type=float, default=1.7, help="sensor height of the rendered map poses (with --mesh)")
    ap.add_argument("--min-valid", type=float, default=0.1, help="drop a rendered pose that sees less than this fraction of its pixels")
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--reach", type=float, default=None)
    ap.add_argument("--odom", help="odometry file of the drive")
    ap.add_argument("--particles", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sigma", type=float, nargs=3, default=[0.1, 0.1, 0.02], metavar=("SX", "SY", "STHETA"))
    ap.add_argument("--init", type=float, nargs=3, default=None, metavar=("X", "Y", "THETA"), help="start around a pose (default: uniform)")
    ap.add_argument("--init-sigma", type=float, nargs=3, default=[1.0, 1.0, 0.2])
    ap.add_argument("--sigma-yaw", type=float, default=None)
    ap.add_argument("--eps-yaw", type=float, default=None)
    ap.add_argument("--overlap-min", type=float, default=None)
    ap.add_argument("--resample-fraction", type=float, default=0.5)
    ap.add_argument("--converged-particles", type=int, default=None)
    ap.add_argument("--converge-radius", type=float, default=1.0)
    a = ap.parse_args(argv)
    if not a.build and not a.odom:
        ap.error("give --build (make a map) or --odom (localize a drive)")
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.localization import MonteCarloLocalizer, OverlapMap
    cfg = load_config(a.config)
    map_scans = a.map_scans or a.scans
    if map_scans:
        cfg["scan_folder"] = map_scans
    infer = Infer(cfg)
    mesh = None
    if a.mesh:
        from overlapnet_amd.mesh import TriangleMesh
        mesh = TriangleMesh.from_obj(a.mesh) if a.mesh.lower().endswith(".obj") else TriangleMesh.from_ply(a.mesh)
    try:
        if a.build and mesh is not None:
            from overlapnet_amd.localization import grid_poses
            if a.build == "grid":
                lo, hi = mesh.vertices.min(axis=0), mesh.vertices.max(axis=0)
                poses = grid_poses((lo[0], hi[0]), (lo[1], hi[1]), a.resolution, a.grid_height)
            else:
                _, rows = read_rows(a.build)
                poses = np.stack([grid_poses((x, x), (y, y), a.resolution, a.grid_height, yaw)[0] for x, y, yaw in rows])
                poses[:, 0, 3], poses[:, 1, 3] = rows[:, 0], rows[:, 1]
            mp = OverlapMap.from_mesh(infer, mesh, poses, a.resolution, a.reach, min_valid_fraction=a.min_valid)
            mp.save(a.map)
            print("map of %d rendered frames (%d of %d poses kept), %d x %d cells of %.3g m, %d occupied -> %s"
                  % (mp.n_frames, len(mp.kept), len(poses), mp.nx, mp.ny, mp.resolution, len(mp.occupied_cells), a.map), file=sys.stderr)
            return 0
        if a.build:
            names, poses = read_rows(a.build)
            mp = OverlapMap(infer, names, poses, a.resolution, a.reach)
            mp.save(a.map)
            print("map of %d keyframes, %d x %d cells of %.3g m, %d occupied -> %s"
                  % (mp.n_frames, mp.nx, mp.ny, mp.resolution, len(mp.occupied_cells), a.map), file=sys.stderr)
            return 0
        mp = OverlapMap.load(infer, a.map, mesh) if mesh is not None else OverlapMap.load(infer, a.map)
        if a.scans:
            infer._scan_folder = a.scans          # the drive's scans from here on (the map is cached)
        obs = {k: v for k, v in (("sigma_yaw", a.sigma_yaw), ("eps_yaw", a.eps_yaw), ("overlap_min", a.overlap_min)) if v is not None}
        loc = MonteCarloLocalizer(mp, a.particles, seed=a.seed, resample_fraction=a.resample_fraction,
                                  converged_particles=a.converged_particles, converge_radius=a.converge_radius, **obs)
        if a.init is not None:
            loc.init_around(a.init, a.init_sigma)
        names, odom = read_rows(a.odom)
        for name, o in zip(names, odom):
            e = loc.step(name, o, a.sigma)
            print("%s %.4f %.4f %.5f %.1f %d %d %d %d" % (name, e.x, e.y, e.yaw, e.n_eff, e.frames_scored, e.off_map, e.resampled, e.lost))
        return 0
    finally:
        infer.close()


if __name__ == "__main__":
    sys.exit(main())
