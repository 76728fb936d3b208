"""NumPy statement of the `TsdfOdometry` loop (overlapnet_amd/odometry.py) from the three references it is made
of -- the ray caster (tests/_raycast_ref.py), the fusion (tests/_tsdf_ref.py) and the registration (tests/_icp_ref.py) -- plus the seeded
drive the GPU test tracks.  A scan of the drive is a rendered image of the scene (tests/_render_ref.py); its points are the hit
pixels' vertices, and since each lies on the ray through its pixel's centre, projecting them gives that image back: the statement takes
the rendered images as the projected scans and the oracle's normal map of them.
"""
import functools

import numpy as np

import _icp_ref as I
import _raycast_ref as RC
import _render_ref as R
import _tsdf_ref as T

N_FRAMES, STEP_M, YAW_DEG, CLEARANCE = 12, 0.5, 1.5, 1.0
HW = (32, 360)
VOXEL, TRUNC, MIN_RANGE = 0.2, 0.8, 0.5
ICP = dict(iterations=20, max_dist=2.0, cos_min=0.8, huber=0.2, min_inliers=64)


@functools.lru_cache(maxsize=None)
def drive(seed=0):
    """(true poses (12,4,4), first pose inverse applied: the poses relative to scan 0 (12,4,4)): steps of 0.5 m along a heading that
    turns 1.5 degrees per frame, every position at least 1 m from every box and from the walls."""
    g = np.random.default_rng([seed, 7])
    blo, bhi = R.scene_boxes(0)
    while True:
        x, y, th = g.uniform(CLEARANCE, R.ROOM[0] - CLEARANCE), g.uniform(CLEARANCE, R.ROOM[1] - CLEARANCE), g.uniform(-np.pi, np.pi)
        xs, ys, ths = [x], [y], [th]
        for _ in range(N_FRAMES - 1):
            xs.append(xs[-1] + STEP_M * np.cos(ths[-1]))
            ys.append(ys[-1] + STEP_M * np.sin(ths[-1]))
            ths.append(ths[-1] + np.radians(YAW_DEG))
        xs, ys = np.array(xs), np.array(ys)
        ok = (xs.min() >= CLEARANCE) and (xs.max() <= R.ROOM[0] - CLEARANCE) and (ys.min() >= CLEARANCE) and (ys.max() <= R.ROOM[1] - CLEARANCE)
        ok = ok and not np.any((xs[:, None] > blo[None, :, 0] - CLEARANCE) & (xs[:, None] < bhi[None, :, 0] + CLEARANCE) &
                               (ys[:, None] > blo[None, :, 1] - CLEARANCE) & (ys[:, None] < bhi[None, :, 1] + CLEARANCE))
        if ok:
            break
    world = np.stack([R.pose_at(a, b, R.SENSOR_Z, c) for a, b, c in zip(xs, ys, ths)])
    rel = np.linalg.inv(world[0])[None] @ world
    rel[0] = np.eye(4)
    return world, rel


def volume_box(world0):
    """(lo, hi) of the odometry's volume in the frame of scan 0: the scene's box grown by 1 m, moved into that frame and boxed again."""
    v, _ = R.scene(0)
    lo, hi = v.min(axis=0).astype(np.float64) - 1.0, v.max(axis=0).astype(np.float64) + 1.0
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    c = (np.linalg.inv(world0) @ corners.T).T[:, :3]
    return c.min(axis=0), c.max(axis=0)


@functools.lru_cache(maxsize=None)
def scans(seed=0):
    """(range (12,H,W), vertex (12,H,W,4)) float32: the scene rendered at the drive's true poses by the renderer's statement."""
    world, _ = drive(seed)
    v, t = R.scene(0)
    r = R.render(v, t, world, HW[0], HW[1])
    return r["range"].astype(np.float32), r["vertex"].astype(np.float32)


def clouds(seed=0):
    """The twelve (N_i,4) float32 clouds: the hit pixels' vertices (x, y, z, 1)."""
    rng, vtx = scans(seed)
    return [np.ascontiguousarray(vtx[s][rng[s] > 0], np.float32) for s in range(rng.shape[0])]


def _normals(rng, vtx):
    from oracle import overlapnet_oracle as O
    return O.gen_normal_map(rng, vtx, HW[0], HW[1]).astype(np.float32)


def track(ranges, vertices, lo, hi, trig="svml"):
    """The loop: -> (poses (n,4,4), sources [str]).  Predict, ray-cast at the prediction, register onto the view, fall back to the
    previous scan, then to the prediction; fuse unless the prediction stands."""
    from overlapnet_amd import tsdf
    shape = tsdf.volume_shape(lo, hi, VOXEL)
    d, w = T.fresh(shape)
    origin = np.asarray(lo, np.float64)
    kw = dict(fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)
    poses, sources = [], []
    prev = None
    for s in range(ranges.shape[0]):
        cur = (ranges[s], vertices[s], _normals(ranges[s], vertices[s]))
        if s == 0:
            pose, src = np.eye(4), "first"
        else:
            t_last = poses[-1]
            t_pred = t_last @ (np.linalg.inv(poses[-2]) @ t_last) if s > 1 else t_last.copy()
            view = RC.raycast(d, w, origin, VOXEL, t_pred[None], HW[0], HW[1], np.float32, MIN_RANGE, R.MAX_RANGE, VOXEL, 1.0)
            vr, vv = view["range"][0], view["vertex"][0]
            model = I.register(cur, (vr, vv, _normals(vr, vv)), np.eye(4), **ICP, **kw)
            if model["status"] == 0:
                pose, src = t_pred @ model["pose"], "model"
            else:
                frame = I.register(cur, prev, np.eye(4), **ICP, **kw)
                pose, src = (t_last @ frame["pose"], "frame") if frame["status"] == 0 else (t_pred, "prediction")
        if src != "prediction":
            o = T.integrate(d, w, origin, VOXEL, TRUNC, T.MAX_WEIGHT, ranges[s:s + 1], pose[None], trig=trig, **kw)
            d, w = o["tsdf"], o["weight"]
        poses.append(pose)
        sources.append(src)
        prev = cur
    return np.stack(poses), sources


def distances(poses, truth):
    """(translation [m], rotation [deg]) of every frame from the truth."""
    e = np.array([I.pose_error(p, q) for p, q in zip(poses, truth)])
    return e[:, 0], e[:, 1]
