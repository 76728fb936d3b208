"""NumPy statement of the range-image ICP of `ovn_icp_register` ("Loop-closure verification"), the reference of
tests/test_icp_host.py and tests/test_gpu_icp.py.  fp64 by default; `arith=np.float32` evaluates the per-point arithmetic (transform,
projection, gates, residual, weight, Jacobian) in float32 like the kernel, with the pose and the sums still fp64 -- the GPU tests
take their tolerance from the distance between the two.  The maps are inputs: the GPU tests pass the ones the GPU used."""
import numpy as np

TRI = [(i, j) for i in range(6) for j in range(i, 6)]          # order of the 21 entries of A in `system`


def rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def make_pose(yaw_deg, t):
    T = rz(yaw_deg)
    T[:3, 3] = t
    return T


def pose_error(T, T_ref):
    """(translation distance [m], rotation angle [deg]) between two poses."""
    d = np.linalg.inv(T_ref) @ T
    c = np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3])), float(np.degrees(np.arccos(c)))


def se3_exp(xi):
    v, w = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-4:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    T[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ v
    return T


def one_pass(src, tgt, T, fov_up=3.0, fov_down=-25.0, max_range=50.0, max_dist=2.0, cos_min=0.8, huber=0.2, arith=np.float64,
             detail=False, shift=(0, 0)):
    """One pass at the pose T.  src / tgt: (range (H,W), vertex (H,W,4), normal (H,W,3)).  Returns a dict with A (6,6), b (6), e,
    count, valid; with detail=True also the per-source-pixel quantities the GPU tests need to bound what a flipped association
    or gate can change (all fp64 unless arith says otherwise): among them KA (N,21) / Kb (N,6), the row w J_k J_l / w J_k r a point
    adds if its distance and angle gates let it.  shift = (du, dv) associates every point with the pixel NEXT to its own (columns
    wrap), the one a point on a pixel border may fall into instead."""
    F = arith
    rs, vs, ns = (np.asarray(a) for a in src)
    rt, vt, nt = (np.asarray(a) for a in tgt)
    H, W = rt.shape
    sel = np.flatnonzero(rs.reshape(-1) > 0)
    p = vs.reshape(-1, 4)[sel, :3].astype(F)
    n_s = ns.reshape(-1, 3)[sel].astype(F)
    R, t = T[:3, :3].astype(F), T[:3, 3].astype(F)
    q_ = p @ R.T + t
    x, y, z = q_[:, 0], q_[:, 1], q_[:, 2]
    d = np.sqrt(x * x + y * y + z * z)
    with np.errstate(all="ignore"):
        in_range = (d > 0) & (d < F(max_range))
        down = F(abs(fov_down) / 180.0 * np.pi)
        inv_fov = F(1.0 / (abs(fov_down) / 180.0 * np.pi + abs(fov_up) / 180.0 * np.pi))
        yaw = -np.arctan2(y, x)
        pitch = np.arcsin(np.clip(z / np.where(in_range, d, 1), -1, 1).astype(F))
        uf = F(0.5) * (yaw * F(1.0 / np.pi) + F(1.0)) * F(W)
        vf = (F(1.0) - (pitch + down) * inv_fov) * F(H)
    u = (np.clip(np.floor(uf), 0, W - 1).astype(np.int64) + shift[0]) % W
    v = np.floor(vf) + shift[1]
    in_fov = (v >= 0) & (v < H)
    pix = np.where(in_fov, v, 0).astype(np.int64) * W + u
    has_t = rt.reshape(-1)[pix] > 0
    q = vt.reshape(-1, 4)[pix, :3].astype(F)
    n = nt.reshape(-1, 3)[pix].astype(F)
    n_ok = (n * n).sum(1) < F(1.5)
    diff = q_ - q
    dist2 = (diff * diff).sum(1)
    near = dist2 <= F(max_dist * max_dist)
    s_ok = (n_s * n_s).sum(1) < F(1.5)
    cosv = (n * (n_s @ R.T)).sum(1)
    facing = cosv >= F(cos_min)
    ok = in_range & in_fov & has_t & n_ok & near & s_ok & facing
    r = (n * diff).sum(1)
    ar = np.abs(r)
    with np.errstate(all="ignore"):
        w = np.where(ar <= F(huber), F(1.0), F(huber) / np.where(ar > 0, ar, 1))
    J = np.concatenate([n, np.cross(q_, n)], axis=1)
    Jd, rd, wd = J[ok].astype(np.float64), r[ok].astype(np.float64), w[ok].astype(np.float64)
    out = dict(A=(Jd * wd[:, None]).T @ Jd, b=(Jd * wd[:, None]).T @ rd, e=float((wd * rd * rd).sum()), count=int(ok.sum()),
               valid=int(sel.size))
    if detail:
        loose = (in_range & in_fov & has_t & n_ok & s_ok).astype(np.float64)
        J64, wl = J.astype(np.float64), w.astype(np.float64) * loose
        out.update(KA=np.stack([wl * J64[:, i] * J64[:, j] for i, j in TRI], axis=1), Kb=(wl * r.astype(np.float64))[:, None] * J64)
        out.update(sel=sel, ok=ok, J=J.astype(np.float64), r=r.astype(np.float64), w=w.astype(np.float64), uf=uf, vf=vf, d=d, dist2=dist2,
                   cosv=cosv, in_range=in_range, in_fov=in_fov, has_t=has_t, n_ok=n_ok, s_ok=s_ok, near=near, facing=facing)
    return out


def system_vector(s):
    """The (28,) layout of `system_dev`: A's upper triangle by rows, b, count."""
    return np.concatenate([[s["A"][i, j] for i, j in TRI], s["b"], [float(s["count"])]])


def register(src, tgt, T0, iterations=20, max_dist=2.0, cos_min=0.8, huber=0.2, min_inliers=64, fov_up=3.0, fov_down=-25.0,
             max_range=50.0, arith=np.float64):
    """-> dict(pose (4,4), status, solved, inliers, valid, rms, last_step (|v|, |omega|), system (28,) of the first pass)."""
    T = np.array(T0, dtype=np.float64)
    kw = dict(fov_up=fov_up, fov_down=fov_down, max_range=max_range, max_dist=max_dist, cos_min=cos_min, huber=huber, arith=arith)
    status, solved, step, system = 0, 0, (0.0, 0.0), None
    for k in range(iterations + 1):
        s = one_pass(src, tgt, T, **kw)
        if k == 0:
            system = system_vector(s)
        if s["count"] < min_inliers:
            status = 1
            break
        if k == iterations:
            break
        try:
            L = np.linalg.cholesky(s["A"])
        except np.linalg.LinAlgError:
            status = 1
            break
        if not np.all(np.isfinite(L)):
            status = 1
            break
        xi = np.linalg.solve(L.T, np.linalg.solve(L, -s["b"]))
        if not np.all(np.isfinite(xi)):
            status = 1
            break
        T = se3_exp(xi) @ T
        solved += 1
        step = (float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:])))
    rms = float(np.sqrt(max(s["e"], 0.0) / s["count"])) if s["count"] > 0 else 0.0
    return dict(pose=T, status=status, solved=solved, inliers=s["count"], valid=s["valid"], rms=rms, last_step=step, system=system)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def moved_cloud(points, T):
    """The (N,4) float32 cloud with its xyz moved by the 4x4 pose T (fp64 arithmetic, one rounding to float32)."""
    out = np.array(points, dtype=np.float32).reshape(-1, 4).copy()
    out[:, :3] = (out[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return out


# (yaw deg, t [m], offset of the initial yaw [deg]); T_gt = make_pose(yaw, t) maps source points into the target frame
REAL_CASES = [(30.0, (1.0, 0.5, 0.1), 0.4), (-120.0, (2.0, -1.0, 0.0), -0.5), (179.0, (0.5, 0.5, 0.05), 0.5), (10.0, (4.0, 2.0, 0.2), 0.5)]
ROOM_CASES = [(30.0, (1.0, 0.5, 0.1), 0.5), (-170.0, (2.0, -1.0, 0.0), -0.5), (0.0, (0.3, 0.0, 0.0), 1.0)]
ROOM_SHAPES = [(16, 100), (8, 90)]
# 2227 pixels: no multiple of 4 (the kernel's scalar loads, a last group of 3 pixels) and more four-pixel groups (557) than the 512
# threads of a workgroup.  The reference converges on it: 2.7 / 4.5 / 2.2 mm from the truth, 1818-2004 inliers, last step 1e-15 m.
ODD_ROOM_SHAPE = (17, 131)


def room_cloud(T_sensor, n_rays, seed, fov_up=3.0, fov_down=-25.0):
    """Points a sensor at pose T_sensor (sensor frame -> room frame) sees inside a 20 x 12 m box room, floor at z = -1.7 m, ceiling
    at +2.3 m: n_rays random directions inside the vertical field of view, in the SENSOR's frame, (N,4) float32."""
    g = np.random.default_rng(seed)
    az = g.uniform(-np.pi, np.pi, n_rays)
    el = np.radians(g.uniform(fov_down + 0.2, fov_up - 0.2, n_rays))
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1) @ T_sensor[:3, :3].T
    o = T_sensor[:3, 3]
    lo, hi = np.array([-10.0, -6.0, -1.7]), np.array([10.0, 6.0, 2.3])
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(dirs > 0, (hi - o) / dirs, np.where(dirs < 0, (lo - o) / dirs, np.inf))
    hit = o + dirs * tt.min(axis=1)[:, None]
    local = (hit - o) @ T_sensor[:3, :3]
    return np.concatenate([local, np.ones((n_rays, 1))], axis=1).astype(np.float32)


def room_pair(case, seed=2, n_rays=25000):
    """(target cloud, source cloud, T_gt, T0) of a ROOM case: the target sensor at the origin, the source sensor at T_gt."""
    yaw, t, off = case
    T_gt = make_pose(yaw, t)
    return room_cloud(np.eye(4), n_rays, seed), room_cloud(T_gt, n_rays, seed + 1), T_gt, rz(yaw + off)
