"""NumPy statement of `ovn_tsdf_integrate` and `ovn_tsdf_triangles` (include/ovn_hip.h).

`integrate` in float32 is the definition itself, operation for operation -- what csrc/tsdf.hip must reproduce bit for bit; in float64
it is the reference on the same float32 inputs, and marks the samples whose decisions a rounding could change AMBIGUOUS.
`triangles` is marching tetrahedra in float32 with its own copy of the case table.  Plus the seeded cases the host and the GPU tests
share (`fused_case`): computed once per process.
"""
import functools

import numpy as np

import _render_ref as R

F32 = np.float32

# ambiguity margins of the float64 reference
AMB_PIX, AMB_SDF, AMB_DEPTH = 1e-3, 1e-5, 1e-5

# the six tetrahedra around the diagonal 0-7 (corner c = dx + 2 dy + 4 dz) and, per inside mask of a tetrahedron's four local vertices
# (bit l = vertex l has tsdf < 0), the edges (a, b) whose crossings are the triangles' vertices, three per triangle
TETS = ((0, 1, 3, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 6, 4, 7), (0, 4, 5, 7), (0, 5, 1, 7))
CASES = {
    1: ((0, 1), (0, 2), (0, 3)),
    2: ((1, 0), (1, 3), (1, 2)),
    4: ((2, 0), (2, 1), (2, 3)),
    8: ((3, 0), (3, 2), (3, 1)),
    14: ((0, 1), (0, 3), (0, 2)),
    13: ((1, 0), (1, 2), (1, 3)),
    11: ((2, 0), (2, 3), (2, 1)),
    7: ((3, 0), (3, 1), (3, 2)),
    3: ((0, 2), (0, 3), (1, 3), (0, 2), (1, 3), (1, 2)),
    5: ((0, 3), (0, 1), (2, 1), (0, 3), (2, 1), (2, 3)),
    9: ((0, 1), (0, 2), (3, 2), (0, 1), (3, 2), (3, 1)),
    6: ((1, 0), (1, 3), (2, 3), (1, 0), (2, 3), (2, 0)),
    10: ((1, 2), (1, 0), (3, 0), (1, 2), (3, 0), (3, 2)),
    12: ((2, 0), (2, 1), (3, 1), (2, 0), (3, 1), (3, 0)),
}


def fresh(shape_xyz):
    nx, ny, nz = shape_xyz
    return np.ones((nz, ny, nx), F32), np.zeros((nz, ny, nx), F32)


def _angles(q0, q1, s, dtype, trig):
    """yaw = -arctan2(y, x), pitch = arcsin(z / depth) the way the mode evaluates them."""
    if dtype is np.float64:
        return -np.arctan2(q1, q0), np.arcsin(s)
    if trig == "svml":
        from oracle import build_oracle as B
        return -B.svml_arctan2(q1, q0), B.svml_arcsin(s)
    if trig == "f64":
        return (-np.arctan2(q1.astype(np.float64), q0.astype(np.float64))).astype(F32), np.arcsin(s.astype(np.float64)).astype(F32)
    raise ValueError("trig must be 'svml' or 'f64'")


def integrate(tsdf, weight, origin, voxel, trunc, max_weight, ranges, poses, fov_up=R.FOV_UP, fov_down=R.FOV_DOWN,
              max_range=R.MAX_RANGE, dtype=np.float32, trig="svml", ambiguous=False, index_offset=(0, 0, 0)):
    """-> dict(tsdf, weight (nz,ny,nx) dtype, updated (n,nz,ny,nx) bool: the scans that changed each sample[, ambiguous (nz,ny,nx)]).
    The inputs are rounded to float32 first in either dtype; `tsdf` and `weight` are not modified.
    index_offset (i0, j0, k0): `tsdf` / `weight` are the block of a larger volume that starts at sample (i0, j0, k0) of it -- its
    sample (i, j, k) sits at origin + (i0 + i, j0 + j, k0 + k) * voxel.  (0, 0, 0) is the statement itself."""
    dt = np.dtype(dtype).type
    nz, ny, nx = tsdf.shape
    t, w = tsdf.astype(dt), weight.astype(dt)
    org = np.asarray(origin, np.float64).astype(F32).astype(dt)
    vox, tr, mw, lim = (dt(F32(v)) for v in (voxel, trunc, max_weight, max_range))
    rng = np.asarray(ranges, F32)
    n, H, W = rng.shape
    up, down = fov_up / 180.0 * np.pi, fov_down / 180.0 * np.pi
    fda, fov = dt(F32(abs(down))), dt(F32(abs(down) + abs(up)))
    with np.errstate(over="ignore", invalid="ignore"):
        P = np.asarray(poses, np.float64).astype(F32)
    i0, j0, k0 = (int(v) for v in index_offset)
    k, j, i = np.meshgrid(np.arange(nz) + k0, np.arange(ny) + j0, np.arange(nx) + i0, indexing="ij")
    p = [org[a] + idx.astype(dt) * vox for a, idx in enumerate((i, j, k))]
    updated = np.zeros((n, nz, ny, nx), bool)
    amb = np.zeros((nz, ny, nx), bool)
    one, zero = dt(1), dt(0)
    for s in range(n):
        if not np.isfinite(P[s, :3, :]).all():
            continue
        Rm, o = P[s, :3, :3].astype(dt), P[s, :3, 3].astype(dt)
        with np.errstate(all="ignore"):
            d = [p[a] - o[a] for a in range(3)]
            q = [(Rm[0, c] * d[0] + Rm[1, c] * d[1]) + Rm[2, c] * d[2] for c in range(3)]
            depth = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
            ok = depth > 0
            safe = np.where(ok, depth, one)
            yaw, pitch = _angles(q[0], q[1], np.where(ok, q[2] / safe, zero), dt, trig)
            px = dt(0.5) * (yaw / dt(F32(np.pi)) + one)
            py = one - (pitch + fda) / fov
            px = px * dt(W)
            py = py * dt(H)
            ok2 = ok & (py >= 0) & (py < dt(H))
            col = np.fmax(zero, np.fmin(dt(W - 1), np.floor(px))).astype(np.int64)
            row = np.where(ok2, np.floor(py), zero).astype(np.int64)
            r = rng[s][row, col].astype(dt)
            ok3 = ok2 & (r > 0) & (r < lim)
            sdf = r - depth
            ok4 = ok3 & ~(sdf < -tr)
            dv = np.fmin(one, sdf / tr)
            w1 = w + one
            tn = (w * t + dv) / w1
            t = np.where(ok4, tn, t)
            w = np.where(ok4, np.fmin(w1, mw), w)
        updated[s] = ok4
        if ambiguous:
            near_int = lambda v: np.abs(v - np.round(v)) < AMB_PIX
            in_rows = ok & (py > -AMB_PIX) & (py < H + AMB_PIX)
            amb |= np.abs(depth) < AMB_DEPTH
            amb |= in_rows & (near_int(px) | near_int(py))
            amb |= ok3 & (np.abs(np.abs(sdf) - tr) < AMB_SDF)
    out = {"tsdf": t, "weight": w, "updated": updated}
    if ambiguous:
        out["ambiguous"] = amb
    return out


def error_bound(origin, shape_xyz, voxel, trunc, poses, n_scans):
    """|tsdf32 - tsdf64| of a sample no decision of which differs, u = 2^-24.  The seven operations: p has two roundings (<= 2 u P per
    coordinate, P the largest |coordinate| of the volume or a sensor), d one and q five more (<= 6 u D each, D the largest depth), the
    square root and its sum three: depth is off by at most sqrt(3) 2 u P + 10 u D.  sdf and dv add two relative roundings of a
    quantity <= 1 after the division by trunc, and every one of the n averaging steps three more of a value <= 1; a weighted mean does
    not amplify the errors of its terms."""
    u = 2.0 ** -24
    org = np.asarray(origin, np.float64)
    far = org + (np.asarray(shape_xyz) - 1) * voxel
    o = np.asarray(poses, np.float64)[:, :3, 3]
    P = max(np.abs(org).max(), np.abs(far).max(), np.abs(o).max())
    corners = np.array([[x, y, z] for x in (org[0], far[0]) for y in (org[1], far[1]) for z in (org[2], far[2])])
    D = max(np.linalg.norm(corners[None] - o[:, None], axis=2).max(), 1.0)
    return (np.sqrt(3.0) * 2 * u * P + 10 * u * D) / trunc + 2 * u + 3 * u * n_scans


# ---- extraction ------------------------------------------------------------------------------------------------------------------
def tet_triangle_count(inside4):
    n = int(sum(inside4))
    return {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n]


def triangles(tsdf, weight, origin, voxel, min_weight=1.0, index_offset=(0, 0, 0)):
    """(T,3,3) float32 in contract order: ascending cell index (x fastest), tetrahedron order, triangle order.
    index_offset (i0, j0, k0): the block of a larger volume, as in `integrate`: vertex coordinates are those of the larger volume
    (the cells of a block keep the larger volume's order: k, then j, then i)."""
    D = np.asarray(tsdf, F32)
    Wt = np.asarray(weight, F32)
    nz, ny, nx = D.shape
    org = np.asarray(origin, np.float64).astype(F32)
    vox = F32(voxel)
    off = [int(v) for v in index_offset]
    corner = lambda a, c: a[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    seen = np.ones((nz - 1, ny - 1, nx - 1), bool)
    inside = np.zeros((8, nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        seen &= corner(Wt, c) >= F32(min_weight)
        inside[c] = corner(D, c) < 0
    live = seen & inside.any(axis=0) & ~inside.all(axis=0)
    ck, cj, ci = np.nonzero(live)                               # ascending linear cell index
    cell = (ck * (ny - 1) + cj) * (nx - 1) + ci
    ins = inside[:, ck, cj, ci]
    keys, verts = [], []
    for t, tet in enumerate(TETS):
        mask = sum(ins[tet[l]].astype(np.int64) << l for l in range(4))
        for m, edges in CASES.items():
            sel = np.nonzero(mask == m)[0]
            if sel.size == 0:
                continue
            pts = []
            for a, b in edges:
                ca, cb = tet[a], tet[b]
                lo, hi = min(ca, cb), max(ca, cb)
                il = [ci[sel] + (lo & 1), cj[sel] + ((lo >> 1) & 1), ck[sel] + (lo >> 2)]
                ih = [ci[sel] + (hi & 1), cj[sel] + ((hi >> 1) & 1), ck[sel] + (hi >> 2)]
                dl, dh = D[il[2], il[1], il[0]], D[ih[2], ih[1], ih[0]]
                f = dl / (dl - dh)
                xyz = []
                for x in range(3):
                    pl = org[x] + (il[x] + off[x]).astype(F32) * vox
                    ph = org[x] + (ih[x] + off[x]).astype(F32) * vox
                    xyz.append(pl + (ph - pl) * f)
                pts.append(np.stack(xyz, -1))
            for qn in range(len(edges) // 3):
                verts.append(np.stack(pts[3 * qn:3 * qn + 3], 1))
                keys.append(np.stack([cell[sel], np.full(sel.size, t), np.full(sel.size, qn)], 1))
    if not verts:
        return np.zeros((0, 3, 3), F32)
    keys, verts = np.concatenate(keys), np.concatenate(verts)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return np.ascontiguousarray(verts[order], F32)


# ---- analytic volumes --------------------------------------------------------------------------------------------------------------
def sphere_volume(n=16, radius=5.3, voxel=0.25, origin=(1.0, -2.0, 0.5)):
    """tsdf = distance to a sphere of `radius` voxels around the volume's centre (in voxels, not truncated), weight 1."""
    c = (n - 1) / 2.0 + 0.13
    k, j, i = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    d = np.sqrt((i - c) ** 2 + (j - c * 0.97) ** 2 + (k - c * 1.02) ** 2) - radius
    centre = np.asarray(origin) + np.array([c, c * 0.97, c * 1.02]) * voxel
    return d.astype(F32), np.ones((n, n, n), F32), np.asarray(origin, np.float64), voxel, centre


def plane_volume(shape_xyz=(11, 9, 7), normal=(0.37, -0.61, 0.70), offset=3.1, voxel=0.5, origin=(-3.0, 2.0, 10.0)):
    nx, ny, nz = shape_xyz
    nrm = np.asarray(normal) / np.linalg.norm(normal)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    d = i * nrm[0] + j * nrm[1] + k * nrm[2] - offset
    return d.astype(F32), np.ones((nz, ny, nx), F32), np.asarray(origin, np.float64), voxel, nrm


def strip_volume():
    """65 x 3 x 3: 256 cells, every one crossed by one of two tilted sheets (tsdf > 0 at j = 0 and 2, < 0 at j = 1) -- the live cells
    run across every workgroup boundary of a compaction whose workgroups own 64 or 128 consecutive cells."""
    k, j, i = np.meshgrid(np.arange(3), np.arange(3), np.arange(65), indexing="ij")
    d = 0.6 * np.cos(np.pi * j) + 0.1 * (k - 1) + 0.003 * i - 0.05
    return d.astype(F32), np.ones((3, 3, 65), F32), np.zeros(3), 0.1, None


ONE_CELL_ORIGIN, ONE_CELL_VOXEL = np.array([2.0, -1.0, 0.5]), 0.5


def one_cell_volumes():
    """[(pattern, inside (8) bool, tsdf (2,2,2) float32)] for the 254 sign patterns of one cell: bit c of the pattern = corner c inside,
    seeded magnitudes in 0.1 .. 1."""
    g = np.random.default_rng(5)
    out = []
    for pattern in range(1, 255):
        inside = np.array([(pattern >> c) & 1 for c in range(8)], bool)
        mag = g.uniform(0.1, 1.0, 8)
        out.append((pattern, inside, np.where(inside, -mag, mag).astype(F32).reshape(2, 2, 2)))
    return out


def unseen_corner_volume():
    """The oblique plane with sample (i, j, k) = (5, 4, 3) seen 0.5 times: (tsdf, weight, origin, voxel, the eight cells around it)."""
    d, w, origin, voxel, _ = plane_volume()
    w = w.copy()
    w[3, 4, 5] = 0.5
    return d, w, origin, voxel, {(i, j, k) for i in (4, 5) for j in (3, 4) for k in (2, 3)}


# ---- the fused cases the host and the GPU tests share --------------------------------------------------------------------------------
# name -> (volume shape (nx,ny,nz), origin in the ROOM's frame, image shape).  Voxel 0.2 m, trunc 0.8 m; box 3 of the seeded scene
# stands 2.5 m from the wall y = 0.
CASES_FUSED = {
    "33x17x9": ((33, 17, 9), None, (16, 90)),
    "70x5x3": ((70, 5, 3), None, (5, 67)),
    "2x2x2": ((2, 2, 2), None, (5, 67)),
    "2x2x2_16x90": ((2, 2, 2), None, (16, 90)),
}
VOXEL, TRUNC, MAX_WEIGHT = 0.2, 0.8, 64.0


def _origins():
    """Volume origins (world frame) from the seeded scene: beside the box nearest to a wall, reaching through that wall."""
    blo, bhi = R.scene_boxes(0)
    gap = np.minimum(blo[:, 1], blo[:, 0])                     # distance of every box to the wall y = 0 or x = 0
    b = int(np.argmin(gap))
    rot = R._rot_z(R.SCENE_ROT)
    at = lambda x, y, z: rot @ np.array([x, y, z])
    if blo[b, 1] <= blo[b, 0]:
        big = at(blo[b, 0] - 1.0, -0.9, -0.3)
        strip = at(blo[b, 0] - 2.0, blo[b, 1] - 0.5, 0.1)
        tiny = at(blo[b, 0] + 0.5, -0.1, 1.0)
    else:
        big = at(-0.9, blo[b, 1] - 1.0, -0.3)
        strip = at(-2.0, blo[b, 1] - 0.5, 0.1)
        tiny = at(-0.1, blo[b, 1] + 0.5, 1.0)
    return {"33x17x9": big, "70x5x3": strip, "2x2x2": tiny, "2x2x2_16x90": tiny}


@functools.lru_cache(maxsize=None)
def scans(H, W, n=5):
    """(ranges (n,H,W) float32, poses (n,4,4)): the first n seeded poses rendered by the NumPy statement of the renderer."""
    v, t = R.scene(0)
    poses = R.scene_poses(n)
    return R.render(v, t, poses, H, W)["range"].astype(F32), poses


@functools.lru_cache(maxsize=None)
def fused_case(name, trig="svml"):
    """dict(shape, origin, ranges, poses, f32 = integrate(float32), f64 = integrate(float64, ambiguous=True)) for a fresh volume."""
    shape, _, (H, W) = CASES_FUSED[name]
    origin = _origins()[name]
    rng, poses = scans(H, W)
    t0, w0 = fresh(shape)
    f32 = integrate(t0, w0, origin, VOXEL, TRUNC, MAX_WEIGHT, rng, poses, dtype=np.float32, trig=trig)
    f64 = integrate(t0, w0, origin, VOXEL, TRUNC, MAX_WEIGHT, rng, poses, dtype=np.float64, ambiguous=True)
    return dict(shape=shape, origin=origin, ranges=rng, poses=poses, f32=f32, f64=f64)
