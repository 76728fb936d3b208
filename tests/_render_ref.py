"""NumPy statement of `ovn_render_scans` (include/ovn_hip.h), twice: in float32 operation for operation -- what the
exhaustive route of csrc/render_mesh.hip must reproduce bit for bit -- and in float64 on the same float32 inputs, with the pixels
whose result a rounding could change marked AMBIGUOUS.  Plus the seeded test scene.  One Python step per TRIANGLE, vectorised over
all rays: fine for the ~10^3 triangles and ~10^5 rays of the tests.
"""
import numpy as np

from overlapnet_amd.mesh import direction_tables

# the sensor of the tests: the reference's field of view, a range short enough that some hits are cut off
FOV_UP, FOV_DOWN, MAX_RANGE = 3.0, -25.0, 20.0
ROOM = (40.0, 30.0, 6.0)
SCENE_ROT = 0.3            # the whole scene is turned about z so that no wall is axis-aligned
SENSOR_Z = 1.7

# ambiguity margins (float64 reference)
AMB_T_REL, AMB_T_ABS, AMB_BARY, AMB_EDGE, AMB_DET = 1.0001, 1e-3, 1e-3, 1e-4, 1e-4


def _grid_quads(origin, du, dv, nu, nv):
    """Triangles of the parallelogram origin + a du + b dv, a, b in [0, 1], split into nu x nv quads of two triangles each."""
    a = np.arange(nu + 1) / nu
    b = np.arange(nv + 1) / nv
    pts = origin[None, None, :] + a[:, None, None] * du[None, None, :] + b[None, :, None] * dv[None, None, :]
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    p00, p10, p01, p11 = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tris = np.concatenate([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)])
    return pts.reshape(-1, 3), tris


def _box_faces(lo, hi):
    d = hi - lo
    ex, ey, ez = np.array([d[0], 0, 0]), np.array([0, d[1], 0]), np.array([0, 0, d[2]])
    return [(lo, ex, ey), (lo + ez, ex, ey), (lo, ex, ez), (lo + ey, ex, ez), (lo, ey, ez), (lo + ex, ey, ez)]


def scene_boxes(seed=0):
    """The twelve boxes (lo, hi) in the room's own frame: 1 - 4 m wide, 0.5 - 3 m tall, standing on the floor, clear of the walls."""
    g = np.random.default_rng([seed, 1])
    size = np.stack([g.uniform(1.0, 4.0, 12), g.uniform(1.0, 4.0, 12), g.uniform(0.5, 3.0, 12)], 1)
    lo = np.stack([g.uniform(1.0, ROOM[0] - 5.0, 12), g.uniform(1.0, ROOM[1] - 5.0, 12), np.zeros(12)], 1)
    return lo, lo + size


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def scene(seed=0):
    """(vertices (V,3) float32, triangles (936,3) int32): a 40 x 30 x 6 m room without ceiling, walls and floor split 6 x 6, twelve
    boxes with faces split 2 x 2, everything turned 0.3 rad about z.  Vertices are not shared between faces."""
    X, Y, Z = ROOM
    o = np.zeros(3)
    ex, ey, ez = np.array([X, 0, 0.0]), np.array([0, Y, 0.0]), np.array([0, 0, Z])
    parts = [_grid_quads(*f, 6, 6) for f in ((o, ex, ey), (o, ex, ez), (o + ey, ex, ez), (o, ey, ez), (o + ex, ey, ez))]
    blo, bhi = scene_boxes(seed)
    for k in range(12):
        parts += [_grid_quads(*f, 2, 2) for f in _box_faces(blo[k], bhi[k])]
    verts, tris, base = [], [], 0
    for p, t in parts:
        verts.append(p)
        tris.append(t + base)
        base += p.shape[0]
    v = np.concatenate(verts) @ _rot_z(SCENE_ROT).T
    return v.astype(np.float32), np.concatenate(tris).astype(np.int32)


def pose_at(x, y, z=SENSOR_Z, yaw=0.0):
    """Sensor pose at (x, y, z) of the ROOM's frame with heading yaw in that frame, as a world (scene) pose."""
    p = np.eye(4)
    p[:3, :3] = _rot_z(SCENE_ROT + yaw)
    p[:3, 3] = _rot_z(SCENE_ROT) @ np.array([x, y, z])
    return p


def scene_poses(n, seed=0):
    """n sensor poses inside the room, outside every box, at height 1.7 m with random yaw."""
    g = np.random.default_rng([seed, 2])
    blo, bhi = scene_boxes(seed)
    out = []
    while len(out) < n:
        x, y, yaw = g.uniform(2.0, ROOM[0] - 2.0), g.uniform(2.0, ROOM[1] - 2.0), g.uniform(-np.pi, np.pi)
        if np.any((x > blo[:, 0] - 0.3) & (x < bhi[:, 0] + 0.3) & (y > blo[:, 1] - 0.3) & (y < bhi[:, 1] + 0.3)):
            continue
        out.append(pose_at(x, y, SENSOR_Z, yaw))
    return np.stack(out)


def box_interior_pose(k, seed=0):
    """A pose in the middle of box k (below its top when the box is taller than the sensor height, else at half its height)."""
    blo, bhi = scene_boxes(seed)
    c = 0.5 * (blo[k] + bhi[k])
    return pose_at(c[0], c[1], c[2], 0.4)


def rays(poses, H, W, dtype, fov_up=FOV_UP, fov_down=FOV_DOWN):
    """(o (n,3), d_s (H,W,3), d_w (n,H,W,3), finite (n)) in `dtype` from the float32 tables and the float32-rounded poses."""
    ca, sa, cp, sp = (t.astype(dtype) for t in direction_tables(H, W, fov_up, fov_down))
    with np.errstate(over="ignore", invalid="ignore"):
        P = np.asarray(poses, np.float64).astype(np.float32)
    R, o = P[:, :3, :3].astype(dtype), P[:, :3, 3].astype(dtype)
    finite = np.isfinite(P[:, :3, :]).all(axis=(1, 2))
    d_s = np.stack([cp[:, None] * ca[None, :], cp[:, None] * sa[None, :], np.broadcast_to(sp[:, None], (H, W))], -1)
    with np.errstate(all="ignore"):
        d_w = np.stack([(R[:, i, 0, None, None] * d_s[None, ..., 0] + R[:, i, 1, None, None] * d_s[None, ..., 1])
                        + R[:, i, 2, None, None] * d_s[None, ..., 2] for i in range(3)], -1)
    return o, d_s, d_w, finite


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _tuv(v, tri, o3, d3, dtype):
    """Moeller-Trumbore of one triangle against all rays: det, u, v, t arrays ((n,H,W)) and the edges."""
    v0, v1, v2 = (v[tri[k]].astype(dtype) for k in range(3))
    e1, e2 = v1 - v0, v2 - v0
    p = _cross(d3, e2)
    det = _dot(e1, p)
    inv = dtype(1) / det
    s = tuple(o3[k] - v0[k] for k in range(3))
    u = _dot(s, p) * inv
    q = _cross(s, e1)
    vv = _dot(d3, q) * inv
    t = _dot(e2, q) * inv
    return det, u, vv, t, e1, e2


def render(vertices, triangles, poses, H, W, dtype=np.float32, max_range=MAX_RANGE, fov_up=FOV_UP, fov_down=FOV_DOWN,
           ambiguous=False):
    """-> dict(range (n,H,W) dtype, tri_id (n,H,W) int32, vertex (n,H,W,4) dtype[, ambiguous (n,H,W) bool]).  dtype float32 is the
    definition itself; float64 is the reference, and `ambiguous` marks the pixels a rounding could change."""
    dtype = np.dtype(dtype).type
    v = np.asarray(vertices, np.float32)
    tris = np.asarray(triangles)
    nv = v.shape[0]
    o, d_s, d_w, finite = rays(poses, H, W, dtype, fov_up, fov_down)
    n = o.shape[0]
    o3 = tuple(o[:, k, None, None] for k in range(3))
    d3 = tuple(d_w[..., k] for k in range(3))
    lim = dtype(np.float32(max_range))
    best_t = np.full((n, H, W), np.inf, dtype)
    best_id = np.full((n, H, W), -1, np.int32)
    ok_pose = finite[:, None, None]
    valid = [i for i in range(tris.shape[0]) if np.all((tris[i] >= 0) & (tris[i] < nv))]
    with np.errstate(all="ignore"):
        for i in valid:
            det, u, vv, t, _, _ = _tuv(v, tris[i], o3, d3, dtype)
            hit = (det != 0) & (det == det) & (u >= 0) & (vv >= 0) & (u + vv <= 1) & (t > 0) & (t < lim) & ok_pose
            better = hit & (t < best_t)          # ascending index: an equal t keeps the earlier triangle
            best_t[better] = t[better]
            best_id[better] = i
    hit = best_id >= 0
    rng = np.where(hit, best_t, dtype(-1))
    vertex = np.full((n, H, W, 4), -1, dtype)
    for k in range(3):
        vertex[..., k] = np.where(hit, rng * d_s[None, ..., k], dtype(-1))
    vertex[..., 3] = np.where(hit, dtype(1), dtype(-1))
    out = {"range": rng, "tri_id": best_id, "vertex": vertex}
    if ambiguous:
        amb = np.zeros((n, H, W), bool)
        t_hi = np.where(hit, AMB_T_REL * best_t + AMB_T_ABS, float(lim) + AMB_T_ABS)
        with np.errstate(all="ignore"):
            for i in valid:
                det, u, vv, t, e1, e2 = _tuv(v, tris[i], o3, d3, dtype)
                cand = (t > 0) & (t <= t_hi) & (u >= -AMB_BARY) & (vv >= -AMB_BARY) & (u + vv <= 1 + AMB_BARY) & ok_pose
                edge = np.minimum(np.minimum(np.abs(u), np.abs(vv)), np.abs(1 - u - vv)) < AMB_EDGE
                flat = np.abs(det) < AMB_DET * np.sqrt(e1 @ e1) * np.sqrt(e2 @ e2)
                cut = np.abs(t - float(lim)) < AMB_T_ABS
                amb |= cand & (edge | flat | cut)
        out["ambiguous"] = amb
    return out


def duplicated(vertices, triangles):
    """The mesh with every triangle listed twice: T + i is a copy of i (the tie rule must report i)."""
    return vertices, np.concatenate([triangles, triangles])
