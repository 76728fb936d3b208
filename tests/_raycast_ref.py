"""NumPy statement of `ovn_tsdf_raycast` and `ovn_tsdf_bricks` (include/ovn_hip.h), twice: in float32 operation
for operation -- what csrc/tsdf_raycast.hip must reproduce bit for bit -- and in float64 on the same float32 inputs, with the pixels
whose result a rounding could change marked AMBIGUOUS.  Vectorised over the rays that are still marching, one Python step per sample k.
Plus the bound on |t*32 - t*64| of a pixel no decision of which differs, and the shared cases of the host and the GPU tests.
"""
import functools
import itertools

import numpy as np

import _render_ref as R
import _tsdf_ref as T

F32 = np.float32
BRICK = 8
MAX_SAMPLES = 1 << 20

# ambiguity margins of the float64 reference
AMB_G, AMB_F = 1e-3, 1e-6


def sample_count(min_range, max_range, step):
    """K: the samples k = 0, 1, .. with min_range + (float)k step < max_range, in float32 (monotone in k)."""
    mn, mx, st = F32(min_range), F32(max_range), F32(step)
    k = max(int((float(mx) - float(mn)) / float(st)) - 2, 0)
    assert k == 0 or mn + F32(k) * st < mx
    while mn + F32(k) * st < mx:
        k += 1
    return k


def bricks(weight, min_weight=1.0):
    """(ceil(nz/8), ceil(ny/8), ceil(nx/8)) uint8: 1 where some sample of the brick has weight >= (float)min_weight."""
    w = np.asarray(weight, F32)
    nz, ny, nx = w.shape
    bz, by, bx = (-(-v // BRICK) for v in (nz, ny, nx))
    ok = np.zeros((bz * BRICK, by * BRICK, bx * BRICK), bool)
    ok[:nz, :ny, :nx] = w >= F32(min_weight)
    return ok.reshape(bz, BRICK, by, BRICK, bx, BRICK).any(axis=(1, 3, 5)).astype(np.uint8)


def _lerp(a, b, f):
    return a + f * (b - a)


def _cell_valid(Wt, mw, fl, shape_xyz, mask, offset=(0, 0, 0)):
    """(in bounds, seen) of the cells with base corner `fl` ((m,3) floats, NaN allowed); `seen` holds for in-bounds cells only.
    offset (i0, j0, k0): Wt (and mask) hold the block of the volume `shape_xyz` that starts there; every sample outside the block is
    unseen, the returned indices are the block's, and "in bounds" then means inside the block (the only cells whose weights
    can sit on the threshold)."""
    nx, ny, nz = shape_xyz
    with np.errstate(invalid="ignore"):
        inb = ((fl[:, 0] >= 0) & (fl[:, 0] <= nx - 2) & (fl[:, 1] >= 0) & (fl[:, 1] <= ny - 2) & (fl[:, 2] >= 0) & (fl[:, 2] <= nz - 2))
    c = np.where(inb[:, None], fl, 0).astype(np.int64) - np.asarray(offset, np.int64)[None, :]
    bz, by, bx = Wt.shape
    inblock = inb & (c[:, 0] >= 0) & (c[:, 0] <= bx - 2) & (c[:, 1] >= 0) & (c[:, 1] <= by - 2) & (c[:, 2] >= 0) & (c[:, 2] <= bz - 2)
    c = np.where(inblock[:, None], c, 0)
    i, j, k = c[:, 0], c[:, 1], c[:, 2]
    seen = inblock.copy()
    if mask is not None:
        seen &= mask[k >> 3, j >> 3, i >> 3] != 0
    for cn in range(8):
        seen &= Wt[k + (cn >> 2), j + ((cn >> 1) & 1), i + (cn & 1)] >= mw
    return inblock, seen, (i, j, k)


def raycast(tsdf, weight, origin, voxel, poses, H, W, dtype=np.float32, min_range=0.5, max_range=R.MAX_RANGE, step=None,
            min_weight=1.0, mask=None, fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, ambiguous=False, index_offset=(0, 0, 0),
            full_shape=None):
    """-> dict(range (n,H,W) dtype, vertex (n,H,W,4) dtype, denom (n,H,W): F_p - F of a hit[, ambiguous (n,H,W) bool]).  dtype float32
    is the definition itself; float64 is the reference.  mask: a brick mask (the route with bricks_dev) or None.
    index_offset (i0, j0, k0) with full_shape (nx, ny, nz): `tsdf` / `weight` (and `mask`) are the block of a volume of full_shape
    that starts at that sample (multiples of 8), the rest of which is unseen (weight below min_weight); the rays are marched through
    the whole volume's index space.  (0, 0, 0) and None are the statement itself."""
    dt = np.dtype(dtype).type
    D, Wt = np.asarray(tsdf, F32), np.asarray(weight, F32)
    nz, ny, nx = D.shape
    shape = (nx, ny, nz) if full_shape is None else tuple(int(v) for v in full_shape)
    off = tuple(int(v) for v in index_offset)
    assert all(v % BRICK == 0 for v in off)
    step = voxel if step is None else step
    K = sample_count(min_range, max_range, step)
    assert 1 <= K <= MAX_SAMPLES
    o, d_s, d_w, finite = R.rays(poses, H, W, dt, fov_up, fov_down)
    n = o.shape[0]
    org = np.asarray(origin, np.float64).astype(F32).astype(dt)
    mn, st, mw = dt(F32(min_range)), dt(F32(step)), F32(min_weight)
    with np.errstate(all="ignore"):
        inv = dt(1) / dt(F32(voxel))
        g_o = np.broadcast_to(((o - org[None, :]) * inv)[:, None, None, :], (n, H, W, 3)).reshape(-1, 3)
        g_d = (d_w * inv).reshape(-1, 3)
    N = n * H * W
    have = np.zeros(N, bool)
    Fp, tp = np.zeros(N, dt), np.zeros(N, dt)
    hit = np.zeros(N, bool)
    t_hit = np.full(N, -1, dt)
    denom = np.zeros(N, np.float64)
    amb = np.zeros(N, bool)
    alive = np.flatnonzero(np.repeat(finite, H * W))
    Dd = D.astype(dt)
    for k in range(K):
        if alive.size == 0:
            break
        t = mn + dt(k) * st
        with np.errstate(all="ignore"):
            g = g_o[alive] + t * g_d[alive]
            fl = np.floor(g)
        inb, valid, (i, j, kk) = _cell_valid(Wt, mw, fl, shape, mask, off)
        F = np.zeros(alive.size, dt)
        v = np.flatnonzero(valid)
        if v.size:
            iv, jv, kv = i[v], j[v], kk[v]
            f = g[v] - fl[v]
            c = [Dd[kv + (cn >> 2), jv + ((cn >> 1) & 1), iv + (cn & 1)] for cn in range(8)]
            with np.errstate(all="ignore"):
                c00, c10, c01, c11 = (_lerp(c[0], c[1], f[:, 0]), _lerp(c[2], c[3], f[:, 0]), _lerp(c[4], c[5], f[:, 0]),
                                      _lerp(c[6], c[7], f[:, 0]))
                c0, c1 = _lerp(c00, c10, f[:, 1]), _lerp(c01, c11, f[:, 1])
                F[v] = _lerp(c0, c1, f[:, 2])
            valid[v] = F[v] == F[v]
        if ambiguous:
            a = np.zeros(alive.size, bool)
            with np.errstate(invalid="ignore"):
                rnd = np.round(g)
                near = np.abs(g - rnd) < AMB_G                                   # (m,3); a NaN is not near
                a |= valid & (np.abs(F) < AMB_F)
            # a coordinate that may fall into the neighbouring cell matters when that cell's validity is another one
            rows = np.flatnonzero(near.any(axis=1))
            if rows.size:
                base_valid = valid[rows]
                other = np.where(fl[rows] == rnd[rows], rnd[rows] - 1, rnd[rows])
                for flip in itertools.product((False, True), repeat=3):
                    if not any(flip):
                        continue
                    use = near[rows] & np.asarray(flip)[None, :]
                    todo = use.any(axis=1) & (use == np.asarray(flip)[None, :]).all(axis=1)
                    if not todo.any():
                        continue
                    alt = np.where(use[todo], other[todo], fl[rows][todo])
                    _, alt_valid, _ = _cell_valid(Wt, mw, alt, shape, None, off)
                    a[rows[todo]] |= alt_valid != base_valid[todo]
            # a corner weight equal to min_weight
            ib = np.flatnonzero(inb)
            if ib.size:
                eq = np.zeros(ib.size, bool)
                for cn in range(8):
                    eq |= Wt[kk[ib] + (cn >> 2), j[ib] + ((cn >> 1) & 1), i[ib] + (cn & 1)] == mw
                a[ib] |= eq
            amb[alive] |= a
        pos = valid & (F > 0)
        end = valid & ~pos
        idx = alive
        cross = end & have[idx]
        if cross.any():
            ci = idx[cross]
            with np.errstate(all="ignore"):
                d = Fp[ci] - F[cross]
                t_hit[ci] = tp[ci] + (t - tp[ci]) * (Fp[ci] / d)
            denom[ci] = d.astype(np.float64)
            hit[ci] = True
        have[idx] = pos
        Fp[idx[pos]] = F[pos]
        tp[idx[pos]] = t
        alive = idx[~end]
    rng = np.where(hit, t_hit, dt(-1)).reshape(n, H, W)
    hit = hit.reshape(n, H, W)
    vertex = np.full((n, H, W, 4), -1, dt)
    with np.errstate(all="ignore"):
        for a_ in range(3):
            vertex[..., a_] = np.where(hit, rng * d_s[None, ..., a_], dt(-1))
    vertex[..., 3] = np.where(hit, dt(1), dt(-1))
    out = {"range": rng, "vertex": vertex, "denom": denom.reshape(n, H, W)}
    if ambiguous:
        out["ambiguous"] = amb.reshape(n, H, W)
    return out


def error_bound(tsdf, origin, voxel, poses, max_range, step, denom):
    """|t*32 - t*64| of a hit pixel no decision of which differs, per pixel from its F_p - F (`denom`, float64 run), u = 2^-24.
    g: g_o has two roundings and inherits one (<= 3 u G, G the largest |grid coordinate| met: the volume's extent plus the sensor's
    distance from its origin, in voxels); d_w has six roundings of terms <= 1 and g_d two more (<= 8 u / voxel), t_k two (2 u T, T =
    max_range), the product and the sum one each: dg <= u (4 G + 11 T / voxel).  F: trilinear in f with slopes <= the largest
    difference dD of neighbouring samples, f = g - floor(g) one rounding, and nine roundings of values <= 2 Dmax in three levels of lerp
    (<= 24 u Dmax): dF <= 3 dD (dg + u) + 24 u Dmax.  The fraction r = F_p / (F_p - F) <= 1 moves by <= 3 dF / denom' + 2 u, denom' =
    denom - 2 dF the smaller of the two runs' denominators; t_p, t_k - t_p, the product and the sum add <= 9 u T."""
    u = 2.0 ** -24
    D = np.asarray(tsdf, np.float64)
    D = np.where(np.isfinite(D), D, 0.0)
    nz, ny, nx = D.shape
    org = np.asarray(origin, np.float64)
    o = np.asarray(poses, np.float64)[:, :3, 3]
    o = o[np.isfinite(o).all(axis=1)]
    Tm = float(max_range)
    G = max(nx, ny, nz) + (np.abs(o - org).max() / voxel if o.size else 0.0) + Tm / voxel
    dg = u * (4 * G + 11 * Tm / voxel)
    dD = max(np.abs(np.diff(D, axis=a)).max() for a in range(3))
    dF = 3 * dD * (dg + u) + 24 * u * np.abs(D).max()
    den = np.maximum(np.asarray(denom, np.float64) - 2 * dF, 1e-300)
    return 9 * u * Tm + float(step) * (3 * dF / den + 3 * u)


# ---- the cases the host and the GPU tests share --------------------------------------------------------------------------------------
IMAGES = ((16, 90), (5, 7))
# min_weight of the shared cases: the weights of these volumes are 0, 0.5 or whole numbers, so 0.75 decides as 1.0 does and no corner
# weight EQUALS it (the float64 reference marks such a corner ambiguous)
MIN_WEIGHT = 0.75


def look_at(eye, target):
    """Sensor pose at `eye` whose x axis (azimuth 0, pitch 0) points at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    x = target - eye
    x /= np.linalg.norm(x)
    up = np.array([0.0, 0.0, 1.0]) if abs(x[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    y = np.cross(up, x)
    y /= np.linalg.norm(y)
    z = np.cross(x, y)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def three_poses(tsdf, weight, origin, voxel):
    """Inside looking out of free space at the surface, outside the volume looking in along the same line (the samples are invalid
    until the ray enters), and one with a NaN.  The line runs from the seen sample with the largest tsdf to the one with the smallest."""
    nz, ny, nx = tsdf.shape
    seen = weight >= 1
    if min(nx, ny, nz) > 2:                                        # keep the free-space end one sample away from the faces
        inner = np.zeros_like(seen)
        inner[1:-1, 1:-1, 1:-1] = True
        seen = seen & inner
    at = lambda flat: np.array(np.unravel_index(flat, tsdf.shape))[::-1].astype(np.float64)      # (i, j, k)
    g_pos = at(np.argmax(np.where(seen, tsdf, -np.inf)))
    g_neg = at(np.argmin(np.where(seen, tsdf, np.inf)))
    line = (g_pos - g_neg) / np.linalg.norm(g_pos - g_neg)
    world = lambda g: np.asarray(origin) + g * voxel
    inside = look_at(world(g_pos - 0.37 * line), world(g_neg))
    far = np.linalg.norm(np.array([nx, ny, nz], np.float64)) + 1.0 / voxel
    outside = look_at(world(g_neg + far * line + np.array([0.21, -0.13, 0.4])), world(g_neg))
    bad = inside.copy()
    bad[1, 2] = np.nan
    return np.stack([inside, outside, bad])


@functools.lru_cache(maxsize=None)
def volume_case(name):
    """dict(tsdf, weight, origin, voxel, poses, max_range, min_range, step) of the named volume."""
    if name == "sphere":
        d, w, origin, voxel, _ = T.sphere_volume()
    elif name == "plane":
        d, w, origin, voxel, _ = T.plane_volume()
    elif name == "one_cell":
        _, _, d = T.one_cell_volumes()[0x0f - 1]                  # the four corners of the face k = 0 inside
        w, origin, voxel = np.ones((2, 2, 2), F32), T.ONE_CELL_ORIGIN, T.ONE_CELL_VOXEL
    elif name == "unseen_corner":
        d, w, origin, voxel, _ = T.unseen_corner_volume()
    elif name == "fused":
        c = T.fused_case("33x17x9")
        d, w, origin, voxel = c["f32"]["tsdf"], c["f32"]["weight"], c["origin"], T.VOXEL
    elif name in EXTRA:
        return _extra_case(name)
    else:
        raise KeyError(name)
    nz, ny, nx = d.shape
    poses = three_poses(d, w, origin, voxel)
    reach = 2.0 * np.linalg.norm((np.array([nx, ny, nz]) - 1) * voxel) + 2.0
    step = 0.25 * voxel if name == "one_cell" else voxel           # one cell holds a single sample of a ray at a step of one voxel
    return dict(tsdf=np.ascontiguousarray(d, F32), weight=np.ascontiguousarray(w, F32), origin=np.asarray(origin, np.float64),
                voxel=float(voxel), poses=poses, min_range=0.3 * voxel, max_range=float(reach), step=float(step))


VOLUMES = ("sphere", "plane", "one_cell", "unseen_corner", "fused")
EXTRA = ("grid_plane", "odd_step", "behind")
CASES = [(v, hw) for v in VOLUMES for hw in IMAGES] + [(e, IMAGES[0]) for e in EXTRA]


def _extra_case(name):
    """The oblique plane again, each with one thing changed."""
    c = dict(volume_case("plane"))
    if name == "grid_plane":
        # a "rotation" whose third row is zero keeps every ray in the plane z = o.z, and o.z is sample plane k = 3 exactly (origin,
        # voxel and the eye are binary fractions): g_z is the integer 3 at every sample, f_z = 0
        P = np.eye(4)
        P[2, 2] = 0.0
        P[:3, 3] = c["origin"] + np.array([8.0, 1.0, 3.0]) * c["voxel"]
        c["poses"] = np.stack([P, P @ np.diag([-1.0, -1.0, 1.0, 1.0])])
    elif name == "odd_step":
        c["step"] = 0.37 * c["voxel"]                               # (max_range - min_range) / step is no whole number
    elif name == "behind":
        # min_range just past the farthest hit of the inside pose: every ray starts in the band behind the surface it never saw
        first = raycast(c["tsdf"], c["weight"], c["origin"], c["voxel"], c["poses"][:1], *IMAGES[0], min_range=c["min_range"],
                        max_range=c["max_range"], step=c["step"], min_weight=MIN_WEIGHT)["range"]
        assert (first > 0).sum() > 100
        c["min_range"] = float(first.max()) + 0.05
        c["poses"] = c["poses"][:1]
    return c


@functools.lru_cache(maxsize=None)
def reference(name, hw, dtype="float32", masked=False):
    """The statement on `volume_case(name)` at image size hw, computed once per process."""
    c = volume_case(name)
    m = bricks(c["weight"], MIN_WEIGHT) if masked else None
    return raycast(c["tsdf"], c["weight"], c["origin"], c["voxel"], c["poses"], hw[0], hw[1], np.dtype(dtype).type, c["min_range"],
                   c["max_range"], c["step"], MIN_WEIGHT, m, ambiguous=(dtype == "float64"))


def stacked(rng, normal, use_depth, use_normals):
    """depth | normals as ovn_render_scans / ovn_tsdf_raycast assemble the leg input."""
    parts = ([rng[..., None]] if use_depth else []) + ([normal] if use_normals else [])
    return np.concatenate(parts, axis=-1)
