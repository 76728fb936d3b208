"""NumPy restatement of the two-flag overlap count of csrc/overlap_gt.hip (gt_pair_kernel) and the inputs its tests share.

The count of a pair needs no range image: per kept point with float32 depth d in pixel p, c = cur[p],
    hit     = d > 0 and |d - c| < 1                       (float32 arithmetic)
    blocked = d <= 0, or d < c and not |d - c| < 1
and the pair's count is #{pixels: some point hits and none blocks}.  `range_image_count` is the definition it must equal:
the count over the pair's float64 range image (oracle.range_image_f64), as com_overlap_yaw.py:40-45 takes it."""
import numpy as np

from oracle import overlapnet_oracle as O

GEOMETRY = dict(fov_up=3.0, fov_down=-25.0, proj_H=64, proj_W=900, max_range=50.0)


def homog(a):
    a = np.asarray(a)
    h = np.ones((a.shape[0], 4), np.float64)
    h[:, :3] = a[:, :3]
    return h


def project(points_xyz1, fov_up=3.0, fov_down=-25.0, proj_H=64, proj_W=900, max_range=50.0):
    """(pixel, float32 depth) of every point the range filter keeps: the arithmetic of oracle.range_image_f64."""
    p = np.asarray(points_xyz1, np.float64)
    up, down = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fov = abs(down) + abs(up)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    depth = np.sqrt((x * x + y * y) + z * z)
    keep = (depth > 0) & (depth < max_range)
    x, y, z, depth = x[keep], y[keep], z[keep], depth[keep]
    px = 0.5 * (-np.arctan2(y, x) / np.pi + 1.0) * proj_W
    py = (1.0 - (np.arcsin(z / depth) + abs(down)) / fov) * proj_H
    px = np.maximum(0, np.minimum(proj_W - 1, np.floor(px))).astype(np.int64)
    py = np.maximum(0, np.minimum(proj_H - 1, np.floor(py))).astype(np.int64)
    return py * proj_W + px, depth.astype(np.float32)


def two_flag_count(pix, d32, cur_flat):
    """#{pixels: hit and not blocked}; cur_flat = the current frame's own range image, flattened float32."""
    c = cur_flat[pix]
    near = np.abs(d32 - c) < np.float32(1)
    hit = np.zeros(cur_flat.size, bool)
    blocked = np.zeros(cur_flat.size, bool)
    hit[pix[(d32 > 0) & near]] = True
    blocked[pix[(d32 <= 0) | ((d32 < c) & ~near)]] = True
    return int(np.count_nonzero(hit & ~blocked))


def moved(scan, ref_pose, inv_cur):
    """The reference scan in the current frame: two sequential float64 products (com_overlap_yaw.py:37-39)."""
    world = ref_pose.dot(homog(scan).T).T
    return inv_cur.dot(world.T).T


def pair_counts(scans, poses, frame, **geometry):
    """(two-flag counts (n,), range-image counts (n,), valid_num) of `frame` against every scan."""
    g = dict(GEOMETRY, **geometry)
    cur = O.range_image_f64(homog(scans[frame]), **g)
    inv_cur = np.linalg.inv(poses[frame])
    flags, images = [], []
    for r in range(len(scans)):
        pts = moved(scans[r], poses[r], inv_cur)
        flags.append(two_flag_count(*project(pts, **g), cur.reshape(-1)))
        ref = O.range_image_f64(pts, **g)
        sel = ref > 0
        images.append(int(np.count_nonzero(np.abs(ref[sel] - cur[sel]) < 1)))
    return np.array(flags), np.array(images), int(np.count_nonzero(cur > 0))


def ray_scans():
    """Scans on ONE ray through the middle of a pixel, and poses (identity): scan 0 = the current frame with its point at 10 m;
    scan 1 = three points on that ray, one nearer than cur - 1, one within 1 m, one beyond: the near one wins the pixel, so it
    must NOT count; scan 2 = the within and the beyond point only: counts; scan 3 = the beyond point only: does not."""
    yaw, pitch = np.radians(12.3), np.radians(-9.1)
    u = np.array([np.cos(pitch) * np.cos(yaw), np.cos(pitch) * np.sin(yaw), np.sin(pitch), 0.0])

    def scan(*ranges):
        return np.array([u * r for r in ranges], np.float32)

    scans = [scan(10.0), scan(8.5, 10.2, 12.0), scan(10.2, 12.0), scan(12.0)]
    return scans, np.stack([np.eye(4)] * len(scans)), np.array([1, 0, 1, 0])


def ragged_scans(fixture, seed=0):
    """Six small scans for the small-geometry cases: an empty one, a one-point one, a 257-point one (one point past a block of
    256 threads), one with (0, 0, 0) and points beyond max_range, and two cuts of the fixture scans; poses on a short curve."""
    rng = np.random.default_rng(seed)
    a, b = fixture["points_0"], fixture["points_1"]
    far = np.array([[0, 0, 0, 0], [60, 5, 1, 0], [0, -80, 2, 0], [49.9, 0, 0, 0], [35.4, 35.4, 0, 0]], np.float32)
    scans = [a[:3000], np.zeros((0, 4), np.float32), b[1234:1235], a[5000:5257],
             np.concatenate([far, b[:700], far[::-1]]), b[-3000:]]
    poses = []
    for i in range(len(scans)):
        ang = 0.2 * i
        T = np.eye(4)
        T[:3, :3] = [[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]
        T[:3, 3] = [0.7 * i, 0.1 * i * i, 0.01 * i] + rng.normal(0, 0.01, 3)
        poses.append(T)
    return [np.ascontiguousarray(s, np.float32) for s in scans], np.stack(poses)


def translation_pairs(n=2000, seed=0):
    """n pairs of poses with the SAME rotation (straight driving): the relative yaw is 0 up to rounding, +-1e-16, which puts
    the scalar yaw bin on the boundary between 179 and 180."""
    rng = np.random.default_rng(seed)
    poses = []
    for _ in range(n):
        ang = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
        for _k in range(2):
            T = np.eye(4)
            T[:3, :3] = R
            T[:3, 3] = rng.uniform(-100, 100, 3)
            poses.append(T)
    return np.stack(poses)
