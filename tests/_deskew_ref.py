"""NumPy statement of `ovn_deskew` (include/ovn_hip_deskew.h), twice -- in float64 (the reference) and in the
header's float32 operation order (for error bounds, not for bits: the device's sine is its own) -- the SE(3) exponential and logarithm
in float64, the azimuth time source, and a generator of BENT scans: scans of the test scene (tests/_render_ref.py) taken by a sensor
that moves while it sweeps.

The generator renders the scene at S poses T_ref Exp((s_j - t_ref) xi), s_j = (j + 1/2) / S, and keeps block j of the image's columns
from render j: a sweep under piecewise-constant motion.  Every point comes with its time s_j and with its hit in the world,
T(s_j) p, so a deskew with the true twist and times is exact up to rounding, not up to a motion model.
"""
import functools

import numpy as np

import _odometry_ref as OD
import _render_ref as R

U = 2.0 ** -24                   # the unit roundoff of float32
SERIES_BELOW_F32 = 2.0 ** -6     # the header's step 3
# float32 error of the azimuth route's time fraction away from the seam, in the header's order: atan2f within 2 ulp of a value below 4
# (8 U in yaw, 8 U / pi = 2.55 U in q) + (float)pi's own error (0.47 U) + the division (1 U) + the addition of 1 (a value below 2:
# 1 U), halved (2.51 U in c), + the rounding of c0, of the difference and of d + 1 for a negative d (0.5 U each): 4.01 U
AZIMUTH_DELTA_S = 4.1 * U


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _coefficients(th):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3) of an array th >= 0 in float64; the series below 0.1."""
    th = np.asarray(th, np.float64)
    t2 = th * th
    small = th < 0.1
    safe = np.where(small, 1.0, th)
    sh = np.sin(0.5 * safe)
    a = np.where(small, 1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110)))), np.sin(safe) / safe)
    b = np.where(small, 0.5 * (1 - t2 / 12 * (1 - t2 / 30 * (1 - t2 / 56 * (1 - t2 / 90 * (1 - t2 / 132))))), 2 * sh * sh / (safe * safe))
    c = np.where(small, (1 - t2 / 20 * (1 - t2 / 42 * (1 - t2 / 72 * (1 - t2 / 110 * (1 - t2 / 156))))) / 6,
                 (safe - np.sin(safe)) / (safe * safe * safe))
    return a, b, c


def se3_exp(xi):
    """Exp of a twist (v, omega) as a 4 x 4 matrix."""
    xi = np.asarray(xi, np.float64).reshape(6)
    v, w = xi[:3], xi[3:]
    a, b, c = (float(x) for x in _coefficients(np.sqrt(w @ w)))
    k = _hat(w)
    t = np.eye(4)
    t[:3, :3] = np.eye(3) + a * k + b * (k @ k)
    t[:3, 3] = v + b * (k @ v) + c * (k @ (k @ v))
    return t


def se3_log(t):
    """The twist (v, omega) of a transform whose rotation angle is below pi."""
    t = np.asarray(t, np.float64)
    r, p = t[:3, :3], t[:3, 3]
    s = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    sn = np.sqrt(s @ s)
    th = np.arctan2(sn, 0.5 * (np.trace(r) - 1.0))
    w = s * (th / sn) if sn > 1e-8 else s
    t2 = th * th
    d = (1 + t2 / 60 * (1 + t2 / 42 * (1 + t2 / 40 * (1 + t2 * 10 / 396)))) / 12 if th < 0.1 else (1 - 0.5 * th / np.tan(0.5 * th)) / t2
    k = _hat(w)
    return np.concatenate([p - 0.5 * (k @ p) + d * (k @ (k @ p)), w])


def _copied(twist):
    twist = np.asarray(twist, np.float64).reshape(6)
    return bool(np.all(twist == 0.0) or not np.isfinite(twist).all())


def deskew(points, times, twist, t_ref):
    """The float64 reference of one scan: points (N,4) float32, times (N,) -> (N,4) float64.  p' = Exp((s - t_ref) xi) p with t_ref
    the float32 the header rounds it to; a zero or non-finite twist copies; a non-finite time gives (0, 0, 0, intensity)."""
    pts = np.asarray(points, np.float32).astype(np.float64)
    if _copied(twist):
        return pts
    xi = np.asarray(twist, np.float64).reshape(6)
    v, w = xi[:3], xi[3:]
    s = np.asarray(times, np.float64)
    good = np.isfinite(s)
    tau = np.where(good, s, 0.0) - float(np.float32(t_ref))
    th = np.sqrt(w @ w)
    a, b, c = _coefficients(np.abs(tau) * th)                     # of the angle |tau| th; K below carries tau's sign
    p = pts[:, :3]
    kp = np.cross(tau[:, None] * w[None], p)
    kkp = np.cross(tau[:, None] * w[None], kp)
    tv = tau[:, None] * v[None]
    kv = np.cross(tau[:, None] * w[None], tv)
    kkv = np.cross(tau[:, None] * w[None], kv)
    out = pts.copy()
    out[:, :3] = (p + a[:, None] * kp + b[:, None] * kkp) + (tv + b[:, None] * kv + c[:, None] * kkv)
    out[~good, :3] = 0.0
    return out


def deskew_f32(points, times, twist, t_ref):
    """The header's operation sequence in float32 with NumPy's sine -> (N,4) float32."""
    f = np.float32
    pts = np.asarray(points, np.float32)
    if _copied(twist):
        return pts.copy()
    xi = np.asarray(twist, np.float64).reshape(6)
    v64, w64 = xi[:3], xi[3:]
    th64 = np.sqrt((w64[0] * w64[0] + w64[1] * w64[1]) + w64[2] * w64[2])
    k64 = w64 / th64 if th64 > 0 else np.zeros(3)
    kv64 = np.cross(k64, v64)
    kkv64 = np.cross(k64, kv64)
    th, k, v, kv, kkv = f(th64), k64.astype(f), v64.astype(f), kv64.astype(f), kkv64.astype(f)
    s = np.asarray(times, np.float32)
    good = np.isfinite(s)
    with np.errstate(all="ignore"):
        tau = np.where(good, s, f(0)) - f(t_ref)
        a = tau * th
        sa = np.sin(a)
        sh = np.sin(f(0.5) * a)
        c1 = (f(2) * sh) * sh
        aa = a * a
        small = np.abs(a) < f(SERIES_BELOW_F32)
        safe = np.where(small, f(1), a)
        B = np.where(small, a * (f(0.5) - aa / f(24)), c1 / safe)
        C = np.where(small, aa * ((f(1) / f(6)) - aa / f(120)), (a - sa) / safe)
        p = [pts[:, i] for i in range(3)]
        cross = lambda q, r: [q[1] * r[2] - q[2] * r[1], q[2] * r[0] - q[0] * r[2], q[0] * r[1] - q[1] * r[0]]
        kp = cross(k, p)
        kkp = cross(k, kp)
        out = pts.copy()
        for i in range(3):
            r = (p[i] + sa * kp[i]) + c1 * kkp[i]
            u = (v[i] + B * kv[i]) + C * kkv[i]
            out[:, i] = r + tau * u
    assert out.dtype == np.float32 and a.dtype == np.float32 and B.dtype == np.float32
    out[~good, :3] = 0.0
    return out


def bound_scale(points, times, twist, t_ref):
    """(|p| + |tau| |v|, |a|) per point: what the kernel's error bound k 2^-24 (|p| + |tau| |v|) scales with, and the angle."""
    xi = np.asarray(twist, np.float64).reshape(6)
    p = np.asarray(points, np.float64)[:, :3]
    tau = np.nan_to_num(np.asarray(times, np.float64), nan=0.0, posinf=0.0, neginf=0.0) - float(np.float32(t_ref))
    return np.sqrt((p * p).sum(1)) + np.abs(tau) * np.sqrt(xi[:3] @ xi[:3]), np.abs(tau) * np.sqrt(xi[3:] @ xi[3:])


def kernel_k(a_max):
    """The k of the bound k 2^-24 (|p| + |tau| |v|) per coordinate for angles |a| <= a_max, counted to first order from the header's
    operation sequence with sinf within 2 ulp (tests/test_gpu_deskew.py carries the count): the larger of the |p| coefficient
    3 + 14 |a| + 12.625 a^2 and the |tau||v| coefficient 10 + 13 |a| + 3.34 a^2."""
    return max(3 + 14 * a_max + 12.625 * a_max ** 2, 10 + 13 * a_max + 3.34 * a_max ** 2)


def azimuth_times(points, start_azimuth_deg, clockwise):
    """The azimuth route's time fractions in float64: yaw = -atan2(y, x), c = (yaw / pi + 1) / 2, c0 likewise from the start azimuth,
    d = c - c0 (clockwise) or c0 - c, s = d - floor(d)."""
    p = np.asarray(points, np.float64)
    c = 0.5 * (-np.arctan2(p[:, 1], p[:, 0]) / np.pi + 1.0)
    c0 = 0.5 * (float(start_azimuth_deg) / 180.0 + 1.0)
    d = c - c0 if clockwise else c0 - c
    return d - np.floor(d)


# ---- bent scans ---------------------------------------------------------------------------------------------------------------------
def slice_times(S):
    """(j + 1/2) / S rounded to float32, as float64: the poses are taken at exactly the times the points are handed over with."""
    return ((np.arange(S) + 0.5) / S).astype(np.float32).astype(np.float64)


def slice_poses(pose_ref, twist, S, t_ref=0.5):
    """(S,4,4): the sensor at the S slice times, T_ref Exp((s_j - t_ref) xi)."""
    return np.stack([np.asarray(pose_ref, np.float64) @ se3_exp((s - t_ref) * np.asarray(twist, np.float64)) for s in slice_times(S)])


def assemble(ranges, vertices, poses):
    """One bent scan from S full renders (S,H,W) / (S,H,W,4) at `poses`: block j of the columns from render j ->
    (points (N,4) float32, times (N,) float32, world hits (N,3) float64), in row-major pixel order."""
    S, H, W = ranges.shape
    pts, tms, hits = [], [], []
    col = np.arange(W)
    owner = np.minimum(col * S // W, S - 1)
    times = slice_times(S)
    for j in range(S):
        mask = (ranges[j] > 0) & (owner[None, :] == j)
        p = np.ascontiguousarray(vertices[j][mask], np.float32)
        pts.append(p)
        tms.append(np.full(p.shape[0], times[j], np.float32))
        p64 = p.astype(np.float64)
        p64[:, 3] = 1.0
        hits.append((poses[j] @ p64.T).T[:, :3])
    return np.concatenate(pts), np.concatenate(tms), np.concatenate(hits)


def bent_scan(pose_ref, twist, H=16, W=180, S=6, t_ref=0.5, render=None):
    """A bent scan of the test scene -> (points, times, world hits).  render(poses) -> (range (S,H,W), vertex (S,H,W,4)); by default
    the renderer's NumPy statement."""
    poses = slice_poses(pose_ref, twist, S, t_ref)
    if render is None:
        v, t = R.scene(0)
        out = R.render(v, t, poses, H, W)
        rng, vtx = out["range"], out["vertex"]
    else:
        rng, vtx = render(poses)
    return assemble(np.asarray(rng, np.float32), np.asarray(vtx, np.float32), poses)


KERNEL_TWIST = np.array([0.9, -0.3, 0.05, 0.01, -0.02, 0.08])        # the twist of the 16 x 180 bent scan of the kernel tests


@functools.lru_cache(maxsize=None)
def kernel_scan():
    """(pose_ref, twist, points, times, world hits) of the 16 x 180, S = 6 bent scan the kernel tests share."""
    pose = R.scene_poses(1)[0]
    return (pose, KERNEL_TWIST) + bent_scan(pose, KERNEL_TWIST)


# The drive of the odometry tests.  At the 0.5 m and 1.5 degrees per sweep of tests/_odometry_ref.py the restatement of the tracker gains
# nothing from a deskew (every error is at the level the snapshot scans reach), so the sensor moves twice as fast:
# 1 m and 3 degrees per sweep, the same scene, frame count, image shape, start-pose search and clearances.
DRIVE_SPEED = 2.0
DRIVE_S = 6


@functools.lru_cache(maxsize=None)
def drive(seed=0, speed=DRIVE_SPEED):
    """`_odometry_ref.drive` with its step and its turn per frame multiplied by `speed` -> (world poses (12,4,4), poses relative to
    scan 0); speed 1 gives that drive itself."""
    step, turn = OD.STEP_M * speed, np.radians(OD.YAW_DEG * speed)
    g = np.random.default_rng([seed, 7])
    blo, bhi = R.scene_boxes(0)
    c = OD.CLEARANCE
    while True:
        x, y, th = g.uniform(c, R.ROOM[0] - c), g.uniform(c, R.ROOM[1] - c), g.uniform(-np.pi, np.pi)
        xs, ys, ths = [x], [y], [th]
        for _ in range(OD.N_FRAMES - 1):
            xs.append(xs[-1] + step * np.cos(ths[-1]))
            ys.append(ys[-1] + step * np.sin(ths[-1]))
            ths.append(ths[-1] + turn)
        xs, ys = np.array(xs), np.array(ys)
        ok = (xs.min() >= c) and (xs.max() <= R.ROOM[0] - c) and (ys.min() >= c) and (ys.max() <= R.ROOM[1] - c)
        ok = ok and not np.any((xs[:, None] > blo[None, :, 0] - c) & (xs[:, None] < bhi[None, :, 0] + c) &
                               (ys[:, None] > blo[None, :, 1] - c) & (ys[:, None] < bhi[None, :, 1] + c))
        if ok:
            break
    world = np.stack([R.pose_at(a, b, R.SENSOR_Z, t) for a, b, t in zip(xs, ys, ths)])
    rel = np.linalg.inv(world[0])[None] @ world
    rel[0] = np.eye(4)
    return world, rel


def drive_twists():
    """(12,6): each frame's true step of the drive as its twist (frame 0 takes frame 1's)."""
    world, _ = drive()
    xi = np.zeros((OD.N_FRAMES, 6))
    for k in range(1, OD.N_FRAMES):
        xi[k] = se3_log(np.linalg.inv(world[k - 1]) @ world[k])
    xi[0] = xi[1]
    return xi


def drive_slice_poses(t_ref=0.5):
    """(12 * S,4,4): the slice poses of every frame of the bent drive, frame-major -- what a renderer is asked for."""
    world, _ = drive()
    return np.concatenate([slice_poses(world[k], xi, DRIVE_S, t_ref) for k, xi in enumerate(drive_twists())])


def bent_drive(ranges, vertices, t_ref=0.5):
    """The twelve bent scans from the renders at `drive_slice_poses` ((12 S,H,W), (12 S,H,W,4)) -> [(points, times, world hits)]."""
    poses = drive_slice_poses(t_ref)
    S = DRIVE_S
    return [assemble(np.asarray(ranges[k * S:(k + 1) * S], np.float32), np.asarray(vertices[k * S:(k + 1) * S], np.float32),
                     poses[k * S:(k + 1) * S]) for k in range(OD.N_FRAMES)]
