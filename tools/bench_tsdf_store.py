"""What the brick store behind the rolling TSDF window costs, on section 36's window: 528 x 528 x 120 samples at
0.2 m, holding `tools/bench_render.py`'s seeded height field fused from `--scans` scans around the field's middle.

  follow           one `follow` by 8 voxels along x, four ways: with a store over a window that holds nothing (flags and their read-back,
                   no brick moves), with a store over the fused window (a slab of the height field is paged out, and paged in again
                   on the way back; the scans are fused `--offset` metres off the window's centre, or that slab would be empty), the clear-only shift alone (what the parent's `follow` pays on the device), and the parent's
                   `follow` that meshes the leaving cells.  `follow` reads back from the device, so all but the clear-only shift
                   are wall-clock milliseconds around a synchronised call; there and back are measured as a pair and halved
  paging           ovn_tsdf_window_page_out and _page_in alone, on a 528 x 528 x 192 window of random words (104 544 bricks), at 10^2,
                   10^4 and 10^5 bricks in ascending (z, y, x) order, against `torch`'s copy of the same bytes taking turns with them:
                   HIP events, windows of at least `--min-ms`, `--rounds` rounds, median; bytes moved / time, and the ratio to the copy
  mesh             `mesh()` after a straight drive of `--drive` metres in steps of 1 m: the sweep of window and store, against the
                   parent's pieces plus window on the same drive (wall-clock, the triangle counts are read back)
  track            one `RollingTsdfOdometry.track` frame on that drive with and without the store: wall-clock median over the frames,
                   and over the frames whose window moved

No threshold is set: the figures are the result.  ONE JSON object on stdout.

    python tools/bench_tsdf_store.py > profiles/tsdf_store.json"""
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
from tools.bench_tsdf_window import HEIGHT, Z_LO  # noqa: E402


def _wall(fn, rounds):
    """Wall-clock milliseconds of `fn()` between two synchronisations, `rounds` times -> (median, all)."""
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 4), [round(v, 4) for v in out]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=224, help="quads per side of the source height field")
    ap.add_argument("--scans", type=int, default=16)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--shift", type=int, default=8)
    ap.add_argument("--offset", type=float, default=10.0, help="the follow section fuses its scans this many metres towards -x of the "
                    "window's centre, so that the slab that leaves holds a surface")
    ap.add_argument("--drive", type=float, default=24.0, help="metres of the straight drive of the mesh and track sections")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_store needs the MI355X: there is no CPU path and no figure to report without it")
    from overlapnet_amd import odometry, tsdf
    from overlapnet_amd import tsdf_store as S
    from overlapnet_amd.engine import OvnEngine
    eng = OvnEngine()
    dev = eng.device
    sensor = dict(fov_up=FOV_UP, fov_down=FOV_DOWN, max_range=MAX_RANGE)
    source = make_mesh(a.grid)
    poses = make_poses(a.scans, 1)
    mid = np.array([EXTENT / 2, EXTENT / 2])
    poses[:, :2, 3] = mid + (poses[:, :2, 3] - mid) * (4.0 / EXTENT)
    poses[:, 2, 3] = ground(poses[:, 0, 3], poses[:, 1, 3]) + SENSOR_Z
    ranges = eng.render_scans(source, poses, H, W, want=("range",), **sensor)["range"]
    trunc = tsdf.DEFAULT_TRUNC_VOXELS * a.voxel
    half = MAX_RANGE + trunc + a.voxel + a.shift * a.voxel
    extent = (2 * half, 2 * half, HEIGHT)
    anchor = (0.0, 0.0, Z_LO + HEIGHT / 2)
    try:
        clock = "%d MHz" % torch.cuda.clock_rate(0)
    except Exception as e:                                                      # noqa: BLE001 -- noted, not needed
        clock = "not available (%s)" % type(e).__name__
    out = {"device": torch.cuda.get_device_name(0), "sm_clock_at_start": clock, "voxel": a.voxel, "shift": a.shift, "offset_m": a.offset,
           "scans_fused": a.scans, "timing": {"warmup": a.warmup, "min_ms": a.min_ms, "rounds": a.rounds}}

    # ---- follow by 8 voxels along x --------------------------------------------------------------------------------------------------
    def window(store, fused):
        vol = tsdf.RollingTsdfVolume(eng, extent, a.voxel, anchor=anchor, shift=a.shift, store=store)
        vol.follow(poses[0, :3, 3])
        if fused:                                  # fused from `--offset` metres towards -x of where the window stands: with the sensor
            moved = poses.copy()                   # at the centre nothing it sees reaches the slab at the window's edge (the
            moved[:, 0, 3] -= a.offset             # tracker's margin), and the slab that leaves would be empty
            vol.integrate(ranges, moved, **sensor)
        return vol

    def there_and_back(vol):
        home = vol.base
        away = tuple(b + s for b, s in zip(home, (a.shift, 0, 0)))
        centre = lambda base: np.asarray(vol.anchor) + (np.asarray(base) + np.asarray([n // 2 for n in vol.shape]) + 0.5) * vol.voxel

        def fn():
            assert vol.follow(centre(away)) and vol.follow(centre(home))
        return fn

    follow = {}
    for name, store, fused in (("store_empty_slab", True, False), ("store_height_field_slab", True, True), ("parent_mesh_leaving_cells", None, True)):
        vol = window(store, fused)
        fn = there_and_back(vol)
        for _ in range(a.warmup):
            fn()
        vol.pieces = []
        med, wins = _wall(fn, 4 * a.rounds)
        rec = {"shape": list(vol.shape), "wall_ms_per_follow_median": round(med / 2, 4), "wall_ms_per_pair": wins}
        if store:
            rec["bricks_in_the_store_at_home"] = len(vol.store)
            vol.follow(np.asarray(vol.anchor) + (np.asarray(vol.base) + np.asarray([n // 2 + (a.shift if i == 0 else 0) for i, n in enumerate(vol.shape)]) + 0.5) * vol.voxel)
            rec["bricks_in_the_store_after_one_move"] = len(vol.store)
            rec["bricks_of_a_slab"] = a.shift // 8 * (vol.shape[1] // 8) * (vol.shape[2] // 8)
        else:
            rec["triangles_per_pair"] = int(sum(p.shape[0] for p in vol.pieces) // max(1, 4 * a.rounds))
        follow[name] = rec
        if name == "store_height_field_slab":
            t, w = vol.tsdf.clone(), vol.weight.clone()
            base = vol.base
            away = tuple(b + s for b, s in zip(base, (a.shift, 0, 0)))

            def shift_pair():
                eng.tsdf_window_shift(t, w, base, away)
                eng.tsdf_window_shift(t, w, away, base)
            res = alternating({"clear_only_shift_pair": shift_pair}, a.warmup, a.min_ms, a.rounds)["clear_only_shift_pair"]
            follow["clear_only_shift"] = {"ms_per_shift_median": round(res[0] / 2, 4), "windows_ms_per_pair": res[1]}
            del t, w
        del vol
        torch.cuda.empty_cache()
    out["follow"] = follow

    # ---- page-out and page-in alone ---------------------------------------------------------------------------------------------------
    nx, ny, nz = 528, 528, 192
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    tsdf_w = torch.rand((nz, ny, nx), device=dev, generator=g)
    weight_w = torch.rand((nz, ny, nx), device=dev, generator=g)
    base = (0, 0, 0)
    keys = np.array([(x, y, z) for z in range(nz // 8) for y in range(ny // 8) for x in range(nx // 8)], np.int32)
    paging = {"window": [nx, ny, nz], "bricks_of_the_window": int(keys.shape[0]), "counts": {}}
    for n in (100, 10000, 100000):
        d_keys = torch.from_numpy(keys[:n].copy()).to(dev)
        d_slots = torch.arange(n, dtype=torch.int32, device=dev)
        pool = torch.zeros(n * S.BRICK_WORDS, dtype=torch.float32, device=dev)
        src = torch.rand(n * S.BRICK_WORDS, device=dev, generator=g)
        fns = {"page_out": lambda: S.window_page_out(eng, tsdf_w, weight_w, base, d_keys, d_slots, pool),
               "page_in": lambda: S.window_page_in(eng, tsdf_w, weight_w, base, d_keys, d_slots, src),
               "torch_copy": lambda: pool.copy_(src)}
        res = alternating(fns, a.warmup, a.min_ms, a.rounds)
        nbytes = n * S.BRICK_BYTES
        rec = {"bytes": nbytes}
        for k, (ms, wins) in res.items():
            rec[k] = {"ms_median": round(ms, 5), "ms_min": round(min(wins), 5), "windows_ms": wins,
                      "gigabytes_moved_per_s": round(nbytes / (ms * 1e-3) / 1e9, 2)}
        for k in ("page_out", "page_in"):
            rec[k]["share_of_the_copy_rate"] = round(res["torch_copy"][0] / res[k][0], 4)
        paging["counts"]["%d" % n] = rec
        del d_keys, d_slots, pool, src
    out["paging"] = paging
    del tsdf_w, weight_w
    torch.cuda.empty_cache()

    # ---- a straight drive: the mesh by sweep and one track frame -----------------------------------------------------------------------
    steps = int(a.drive) + 1
    drive = np.repeat(np.eye(4)[None], steps, axis=0)
    drive[:, 0, 3] = mid[0] - a.drive / 2 + np.arange(steps)
    drive[:, 1, 3] = mid[1]
    drive[:, 2, 3] = ground(drive[:, 0, 3], drive[:, 1, 3]) + SENSOR_Z
    views = eng.render_scans(source, drive, H, W, want=("range", "vertex"), **sensor)
    mesh, track = {}, {}
    for name, store in (("store", True), ("parent", None)):
        vol = tsdf.RollingTsdfVolume(eng, extent, a.voxel, anchor=anchor, shift=a.shift, store=store)
        for s in range(steps):
            vol.follow(drive[s, :3, 3])
            vol.integrate(views["range"][s:s + 1], drive[s:s + 1], **sensor)
        vol.mesh()                                                               # warm-up: the allocator has its blocks
        med, wins = _wall(lambda: vol.mesh(), a.rounds)
        mesh[name] = {"shifts": vol.n_shifts, "triangles": vol.mesh().n_triangles, "wall_ms_median": med, "wall_ms": wins,
                      "stored_bricks": len(vol.store) if store else None, "pieces": len(vol.pieces)}
        del vol
        torch.cuda.empty_cache()
        rng, vtx = views["range"].cpu().numpy(), views["vertex"].cpu().numpy()
        clouds = [np.ascontiguousarray(vtx[s][rng[s] > 0], np.float32) for s in range(steps)]
        odo = odometry.RollingTsdfOdometry(eng, extent, a.voxel, anchor=anchor, shift=a.shift, store=store, proj_h=H, proj_w=W,
                                           min_range=MIN_RANGE, **sensor)
        frame, moved = [], []
        for s, c in enumerate(clouds):
            before = odo.volume.base
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            odo.track(c, first_pose=drive[0] if s == 0 else None)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if s >= 2:                                                           # the first frames allocate
                (moved if odo.volume.base != before else frame).append(ms)
        err = float(np.linalg.norm(odo.poses[-1][:3, 3] - drive[-1, :3, 3]))
        track[name] = {"frames_that_stayed": len(frame), "wall_ms_median_stayed": round(float(np.median(frame)), 4),
                       "frames_that_moved": len(moved), "wall_ms_median_moved": round(float(np.median(moved)), 4) if moved else None,
                       "end_position_error_m": round(err, 4), "stored_bricks": len(odo.volume.store) if store else None}
        del odo
        torch.cuda.empty_cache()
    out["mesh"] = dict(mesh, drive_m=a.drive, steps=steps)
    out["track"] = track
    out["not_measured"] = ["a real drive that revisits a street", "a pool near max_bytes", "more than one GPU",
                           "counters: the share of the copy rate is explained from the access pattern, not from a profile"]
    print(json.dumps(out, indent=1))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
