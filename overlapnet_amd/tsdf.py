"""A map's mesh from a drive: range images and poses fused into a truncated signed distance volume on the GPU, and the volume's zero
level set as a `mesh.TriangleMesh` (ovn_tsdf_integrate / ovn_tsdf_triangles, csrc/tsdf.hip).

    vol = TsdfVolume(engine, lo, hi, voxel=0.2)
    vol.integrate_scans(points, offsets, poses)        # or vol.integrate(range_images, poses)
    mesh = vol.mesh()                                  # -> OverlapMap.from_mesh, mesh.to_ply, tools/localize.py --mesh
    views = vol.render_scans(poses)                    # the volume itself seen from poses (ovn_tsdf_raycast)

The volume is dense: (nz, ny, nx) float32 tsdf and weight, at most 2^31 - 1 samples.  Argument errors raise before a GPU is touched.
`RollingTsdfVolume` is the same pair of arrays as a window that follows the sensor over a lattice fixed in the world (ovn_tsdf_window_*;
DESIGN.md section 36).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ._lib import OvnError
from .mesh import MAX_TRIANGLES, TriangleMesh

MAX_SAMPLES = 2 ** 31 - 1
DEFAULT_TRUNC_VOXELS = 4.0


def volume_shape(lo, hi, voxel: float) -> Tuple[int, int, int]:
    """(nx, ny, nz): samples at lo + (i, j, k) * voxel up to the first one at or past hi on every axis (at least 2 per axis).  Raises
    ValueError for bounds that are not 3 finite numbers with lo < hi, a voxel that is not > 0, or a volume over MAX_SAMPLES samples --
    the message then names the voxel size that would fit."""
    lo = np.asarray(lo, np.float64).reshape(-1)
    hi = np.asarray(hi, np.float64).reshape(-1)
    if lo.shape[0] != 3 or hi.shape[0] != 3:
        raise ValueError("lo and hi must hold 3 numbers each, got %d and %d" % (lo.shape[0], hi.shape[0]))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("the bounds must be finite with lo < hi on every axis, got lo %s hi %s" % (lo.tolist(), hi.tolist()))
    voxel = float(voxel)
    if not (voxel > 0.0 and np.isfinite(voxel) and np.float32(voxel) > 0):
        raise ValueError("voxel must be a finite number > 0, got %r" % (voxel,))
    ext = hi - lo
    n = np.maximum(np.ceil(ext / voxel - 1e-9) + 1.0, 2.0)
    if float(np.prod(n)) > MAX_SAMPLES:
        fit = float((np.prod(ext) / MAX_SAMPLES) ** (1.0 / 3.0))
        shown = float("%.3g" % fit)                # the number the message prints must itself fit
        while np.prod(np.maximum(np.ceil(ext / shown - 1e-9) + 1.0, 2.0)) > MAX_SAMPLES:
            fit *= 1.01
            shown = float("%.3g" % fit)
        fit = shown
        raise ValueError("a volume of %s m at voxel %g m has %.3g samples, over the limit of 2^31 - 1: a voxel of %.3g m fits"
                         % (ext.tolist(), voxel, float(np.prod(n)), fit))
    return int(n[0]), int(n[1]), int(n[2])


MAX_RAY_SAMPLES = 1 << 20        # OVN_RAYCAST_MAX_SAMPLES


def ray_samples(min_range: float, max_range: float, step: float) -> int:
    """The number of samples k = 0, 1, .. with t_k = min_range + (float)k * step < max_range, every operation in float32 as the
    kernel evaluates it (t_k does not decrease with k, so the count is the first k that fails)."""
    mn, mx, st = np.float32(min_range), np.float32(max_range), np.float32(step)
    inside = lambda k: bool(mn + np.float32(k) * st < mx)
    if not inside(0):
        return 0
    hi = 1
    while inside(hi):
        hi *= 2
        if hi > 4 * MAX_RAY_SAMPLES:
            return hi
    lo = hi // 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if inside(mid) else (lo, mid)
    return hi


def check_march(min_range: float, max_range: float, step: float) -> int:
    """Raises ValueError for what ovn_tsdf_raycast refuses in its three march parameters; -> the sample count K."""
    with np.errstate(over="ignore"):
        v = [np.float32(float(x)) for x in (min_range, max_range, step)]
    if not all(np.isfinite(x) and x > 0 for x in v):
        raise ValueError("min_range, max_range and step must be finite numbers > 0 in float32, got %r, %r, %r" % (min_range, max_range, step))
    if not v[0] < v[1]:
        raise ValueError("min_range %r is not below max_range %r" % (min_range, max_range))
    k = ray_samples(*v)
    if k > MAX_RAY_SAMPLES:
        raise ValueError("range %r .. %r in steps of %r is more than 2^20 samples per ray" % (min_range, max_range, step))
    return k


class TsdfVolume(object):
    """A dense TSDF over the box lo .. hi.  `trunc` (metres) defaults to 4 voxels; a sample's weight saturates at `max_weight`."""

    def __init__(self, engine, lo, hi, voxel: float, trunc: float = None, max_weight: float = 64.0):
        self.nx, self.ny, self.nz = volume_shape(lo, hi, voxel)
        self.voxel = float(voxel)
        self.trunc = DEFAULT_TRUNC_VOXELS * self.voxel if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        if not (self.trunc > 0.0 and np.isfinite(self.trunc)):
            raise ValueError("trunc must be a finite number > 0, got %r" % (trunc,))
        if not self.max_weight > 0.0:
            raise ValueError("max_weight must be > 0, got %r" % (max_weight,))
        self.origin = np.asarray(lo, np.float64).reshape(3).copy()
        self.engine = engine
        import torch
        shape = (self.nz, self.ny, self.nx)
        self.tsdf = torch.ones(shape, dtype=torch.float32, device=engine.device)
        self.weight = torch.zeros(shape, dtype=torch.float32, device=engine.device)
        self.n_scans = 0

    @property
    def n_samples(self) -> int:
        return self.nx * self.ny * self.nz

    def _window(self) -> dict:
        """What the engine's calls take beyond the dense volume's arguments: nothing (RollingTsdfVolume: its base)."""
        return {}

    def reset(self) -> None:
        """Back to the fresh volume: tsdf = 1, weight = 0."""
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.n_scans = 0

    @staticmethod
    def _check_sensor(max_range: float) -> None:
        if not (float(max_range) > 0.0 and np.isfinite(float(max_range))):
            raise ValueError("max_range must be a finite number > 0, got %r" % (max_range,))

    def integrate(self, range_images, poses, fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0) -> None:
        """Fuses range images ((n,H,W) float32, -1 = empty; device tensor or host array) taken at `poses` ((n,4,4) sensor to world),
        in order.  The images must come from `project` / `render_scans` with the same field of view."""
        import torch
        self._check_sensor(max_range)
        shape = tuple(range_images.shape)
        if len(shape) != 3 or shape[1] < 1 or shape[2] < 1:
            raise ValueError("range_images must be (n,H,W) with H, W >= 1, got %s" % (shape,))
        pshape = tuple(np.shape(poses)) if not isinstance(poses, torch.Tensor) else tuple(poses.shape)
        if pshape != (shape[0], 4, 4):
            raise ValueError("poses must be (%d,4,4) for %d range images, got %s" % (shape[0], shape[0], pshape))
        if shape[0] == 0:
            return
        if isinstance(range_images, torch.Tensor):
            r = range_images.to(self.engine.device, torch.float32).contiguous()
        else:
            r = torch.from_numpy(np.ascontiguousarray(range_images, np.float32)).to(self.engine.device)
        self.engine.tsdf_integrate(self.tsdf, self.weight, self.origin, self.voxel, self.trunc, self.max_weight, r, poses, fov_up,
                                   fov_down, max_range, **self._window())
        self.n_scans += shape[0]

    def integrate_scans(self, points, offsets, poses, proj_h: int = 64, proj_w: int = 900, fov_up: float = 3.0,
                        fov_down: float = -25.0, max_range: float = 50.0, chunk: int = 64, deskew=None, twists=None, times=None) -> None:
        """Projects raw scans -- `points` (total,4) float32 of concatenated scans, `offsets` (n+1) int64 -- with `engine.project` and
        fuses them, `chunk` scans at a time.  deskew: None, or the dict of `deskew.check_config` -- the scans are raw sweeps and each
        chunk is moved into the sensor frames of fraction t_ref (`deskew.deskew_scans`) ahead of its projection,
        under `twists` (n,6), by default `deskew.twists_from_poses(poses)`; `poses` are then the sensor's at t_ref.  times: (total,)
        float32, one fraction per row of `points`, where the dict names no azimuth parameters."""
        import torch
        from . import deskew as _deskew
        cfg = _deskew.check_config(deskew)
        if cfg is None and (twists is not None or times is not None):
            raise ValueError("twists and times belong to deskew=")
        if cfg is not None:
            source = _deskew.source_of(cfg, times, "integrate_scans")
            if times is not None and tuple(times.shape) != (int(points.shape[0]),):
                raise ValueError("integrate_scans: times must hold one fraction per point, (%d,), got %s"
                                 % (int(points.shape[0]), tuple(times.shape)))
        self._check_sensor(max_range)
        offs = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, np.int64).reshape(-1)
        n = offs.shape[0] - 1
        pshape = tuple(np.shape(poses)) if not isinstance(poses, torch.Tensor) else tuple(poses.shape)
        if n < 0 or pshape != (max(n, 0), 4, 4):
            raise ValueError("poses must be (n,4,4) for the n = %d scans of offsets, got %s" % (n, pshape))
        if int(chunk) < 1 or int(proj_h) < 1 or int(proj_w) < 1:
            raise ValueError("chunk, proj_h and proj_w must be >= 1, got %r, %r, %r" % (chunk, proj_h, proj_w))
        if n == 0:
            return
        if np.any(np.diff(offs) < 0) or offs[0] < 0 or offs[-1] > int(points.shape[0]):
            raise ValueError("offsets must ascend within the %d points" % int(points.shape[0]))
        dev = self.engine.device
        pts = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, np.float32))
        pts = pts.to(dev, torch.float32).contiguous()
        d_offs = torch.from_numpy(offs).to(dev)
        poses = poses if isinstance(poses, torch.Tensor) else np.asarray(poses, np.float64)
        if cfg is not None:
            if times is not None:
                source = dict(times=_deskew.times_tensor(self.engine, times, int(pts.shape[0]), "integrate_scans"))
            if twists is None:
                twists = _deskew.twists_from_poses(poses.cpu().numpy() if isinstance(poses, torch.Tensor) else poses)
            if not isinstance(twists, torch.Tensor):
                twists = torch.from_numpy(np.ascontiguousarray(np.asarray(twists, np.float64)))
            if tuple(twists.shape) != (n, 6):
                raise ValueError("twists must be (%d,6) for the %d scans of offsets, got %s" % (n, n, tuple(twists.shape)))
            twists = twists.to(dev, torch.float64).contiguous()
            raw, pts = pts, torch.empty_like(pts)            # every chunk writes its own rows of `pts`, which is never the caller's tensor
        for a in range(0, n, int(chunk)):
            b = min(n, a + int(chunk))
            max_points = int(np.diff(offs[a:b + 1]).max())
            if cfg is not None:
                _deskew.deskew_scans(self.engine, raw, d_offs[a:b + 1], twists[a:b], t_ref=cfg["t_ref"], out=pts, **source)
            r = self.engine.project(pts, d_offs[a:b + 1], max_points, int(proj_h), int(proj_w), fov_up, fov_down, max_range,
                                    want=("range",))["range"]
            self.engine.tsdf_integrate(self.tsdf, self.weight, self.origin, self.voxel, self.trunc, self.max_weight, r, poses[a:b],
                                       fov_up, fov_down, max_range, **self._window())
        self.n_scans += n

    def bricks(self, min_weight: float = 1.0, out=None):
        """The byte mask of the 8 x 8 x 8 bricks that hold a sample with weight >= min_weight (`engine.tsdf_bricks`)."""
        if np.isnan(float(min_weight)):
            raise ValueError("min_weight is NaN")
        return self.engine.tsdf_bricks(self.weight, min_weight, out=out)

    def render_scans(self, poses, proj_h: int = 64, proj_w: int = 900, fov_up: float = 3.0, fov_down: float = -25.0,
                     min_range: float = 0.5, max_range: float = 50.0, step: float = None, min_weight: float = 1.0, bricks=True,
                     want=("range", "normal"), stacked_flags=None, stacked_out=None, out=None):
        """The volume seen from `poses` ((n,4,4) sensor to world): `engine.tsdf_raycast` on this volume, `step` one voxel by default.
        bricks=True builds the brick mask once for this call, False marches without one, a tensor is taken as the mask of
        `bricks(min_weight)` (the caller's to keep current with the volume)."""
        pshape = tuple(poses.shape) if hasattr(poses, "shape") else tuple(np.shape(poses))
        if len(pshape) != 3 or pshape[1:] != (4, 4):
            raise ValueError("poses must be (n,4,4), got %s" % (pshape,))
        step = self.voxel if step is None else float(step)
        check_march(min_range, max_range, step)
        if np.isnan(float(min_weight)):
            raise ValueError("min_weight is NaN")
        if int(proj_h) < 1 or int(proj_w) < 1:
            raise ValueError("proj_h and proj_w must be >= 1, got %r, %r" % (proj_h, proj_w))
        mask = None
        if bricks is True:
            mask = self.bricks(min_weight)
        elif bricks is not False and bricks is not None:
            mask = bricks
        return self.engine.tsdf_raycast(self.tsdf, self.weight, self.origin, self.voxel, poses, int(proj_h), int(proj_w), fov_up,
                                        fov_down, min_range, max_range, step, min_weight, mask, want, stacked_flags, stacked_out, out,
                                        **self._window())

    def triangles(self, min_weight: float = 1.0):
        """(T,3,3) float32 device tensor of the triangle soup, in contract order: one counting call, then one writing call."""
        tri, total = self.engine.tsdf_triangles(self.tsdf, self.weight, self.origin, self.voxel, min_weight)
        if total == 0:
            raise OvnError("TsdfVolume.mesh: no surface: no cell has all eight corners seen %g times and a sign change "
                           "(%d scans fused)" % (min_weight, self.n_scans))
        return tri

    def mesh(self, min_weight: float = 1.0) -> TriangleMesh:
        """The zero level set as a TriangleMesh: a soup, vertices (3T,3) and triangles arange(3T).reshape(T,3)."""
        if np.isnan(float(min_weight)):
            raise ValueError("min_weight is NaN")
        tri = self.triangles(min_weight)
        t = int(tri.shape[0])
        if t > MAX_TRIANGLES:
            raise OvnError("TsdfVolume.mesh: %d triangles exceed the 2^27 a TriangleMesh holds: use a larger voxel" % t)
        return TriangleMesh(tri.reshape(3 * t, 3).cpu().numpy(), np.arange(3 * t, dtype=np.int32).reshape(t, 3))


# ---- a volume that follows the sensor ----------------------------------------------------------------------
WINDOW_MAX_INDEX = 1 << 20       # |lattice index| of every sample of a window: (float)I is exact


def window_shape(extent, voxel: float) -> Tuple[int, int, int]:
    """(nx, ny, nz) of a window `extent` metres wide (3 numbers, or one for all axes): extent / voxel samples, rounded up to a multiple
    of 8, at least 16 per axis.  Raises ValueError for an extent or voxel that is not finite and > 0 or a window over MAX_SAMPLES."""
    ext = np.asarray(extent, np.float64).reshape(-1)
    if ext.shape[0] == 1:
        ext = np.repeat(ext, 3)
    voxel = float(voxel)
    if ext.shape[0] != 3 or not (np.isfinite(ext).all() and (ext > 0).all()):
        raise ValueError("extent must be 1 or 3 finite numbers > 0, got %r" % (extent,))
    if not (voxel > 0.0 and np.isfinite(voxel) and np.float32(voxel) > 0):
        raise ValueError("voxel must be a finite number > 0, got %r" % (voxel,))
    n = np.maximum(np.ceil(np.ceil(ext / voxel - 1e-9) / 8.0) * 8.0, 16.0)
    if float(np.prod(n)) > MAX_SAMPLES:
        raise ValueError("a window of %s m at voxel %g m has %.3g samples, over the limit of 2^31 - 1" % (ext.tolist(), voxel, np.prod(n)))
    return int(n[0]), int(n[1]), int(n[2])


def check_window(shape, base) -> None:
    """Raises ValueError for what the ovn_tsdf_window_* calls refuse in a window's shape (nx, ny, nz) and base."""
    shape, base = [int(v) for v in shape], [int(v) for v in base]
    if len(shape) != 3 or len(base) != 3:
        raise ValueError("a window has 3 dimensions and a base of 3 indices, got %r and %r" % (shape, base))
    if any(n < 16 or n % 8 for n in shape):
        raise ValueError("the dimensions of a window must be multiples of 8 and >= 16, got %s" % (shape,))
    if shape[0] * shape[1] * shape[2] > MAX_SAMPLES:
        raise ValueError("a window of %s samples is over the limit of 2^31 - 1" % (shape,))
    if any(b % 8 for b in base):
        raise ValueError("every component of a window's base must be a multiple of 8, got %s" % (base,))
    if any(b < -WINDOW_MAX_INDEX or b + n - 1 > WINDOW_MAX_INDEX for b, n in zip(base, shape)):
        raise ValueError("the window %s at base %s leaves the lattice indices -2^20 .. 2^20 (moving the anchor is not supported)"
                         % (shape, base))


def leaving_boxes(old_base, new_base, shape):
    """The lattice points of the box old_base .. old_base + shape - 1 that the box of the same shape at new_base does not hold, as at
    most three disjoint boxes [(lo, hi)], hi exclusive: what leaves along x; of the rest what leaves along y; of the rest along z."""
    ob, nb, n = (np.asarray(v, np.int64).reshape(3) for v in (old_base, new_base, shape))
    lo, hi = ob.copy(), ob + n                   # what is left of the old box
    out = []
    for a in range(3):
        keep_lo, keep_hi = max(lo[a], nb[a]), min(hi[a], nb[a] + n[a])
        if keep_lo >= keep_hi:                   # nothing of this axis stays: all that is left leaves
            out.append((lo.copy(), hi.copy()))
            break
        for l, h in ((lo[a], keep_lo), (keep_hi, hi[a])):    # below the new box or above it: a shift leaves one of them empty
            if l < h:
                blo, bhi = lo.copy(), hi.copy()
                blo[a], bhi[a] = l, h
                out.append((blo, bhi))
        lo[a], hi[a] = keep_lo, keep_hi
    return [(tuple(int(v) for v in l), tuple(int(v) for v in h)) for l, h in out if np.all(np.asarray(l) < np.asarray(h))]


class RollingTsdfVolume(TsdfVolume):
    """A TSDF of fixed size whose window follows the sensor (ovn_tsdf_window_*).

        vol = RollingTsdfVolume(engine, extent=(120, 120, 24), voxel=0.2)
        vol.follow(position); vol.integrate(range_images, poses); views = vol.render_scans(poses)
        mesh = vol.mesh()                                  # what left the window on the way, plus the window

    The lattice is fixed: sample (I, J, K) sits at anchor + (I, J, K) * voxel.  The window holds base <= (I, J, K) < base + (nx, ny,
    nz) in ring storage and starts centred on the anchor.  `follow` moves the base in multiples of `shift` voxels (a multiple of 8) and
    meshes the cells that lose a corner before their slots are cleared.  A region the window comes back to is fresh.

    store: None (the default) is all of the above and makes the launches it always made.  True, or a
    `tsdf_store.TsdfBrickStore` (one that `load` made continues a saved map; its voxel, anchor and trunc must be this volume's), keeps
    what leaves: `follow` pages the non-empty 8 x 8 x 8 bricks of the leaving samples out to the store, shifts, and pages the stored
    bricks of the entering samples back in, so a region the window comes back to holds what it held.  `follow` then meshes nothing and
    `mesh()` sweeps window and store, every cell once."""

    store = None                         # the TsdfBrickStore of a volume built with store=

    def __init__(self, engine, extent, voxel: float, trunc: float = None, max_weight: float = 64.0, anchor=(0.0, 0.0, 0.0),
                 shift: int = 8, store=None):
        self.nx, self.ny, self.nz = window_shape(extent, voxel)
        self.voxel = float(voxel)
        self.trunc = DEFAULT_TRUNC_VOXELS * self.voxel if trunc is None else float(trunc)
        self.max_weight = float(max_weight)
        if not (self.trunc > 0.0 and np.isfinite(self.trunc)):
            raise ValueError("trunc must be a finite number > 0, got %r" % (trunc,))
        if not self.max_weight > 0.0:
            raise ValueError("max_weight must be > 0, got %r" % (max_weight,))
        if int(shift) != shift or int(shift) < 8 or int(shift) % 8:
            raise ValueError("shift must be a multiple of 8 voxels, got %r" % (shift,))
        self.shift = int(shift)
        self.origin = np.asarray(anchor, np.float64).reshape(-1).copy()      # the anchor: what the dense calls name origin
        if self.origin.shape[0] != 3 or not np.isfinite(self.origin).all():
            raise ValueError("anchor must be 3 finite numbers, got %r" % (anchor,))
        self.base = tuple(-(n // 2) // 8 * 8 for n in self.shape)
        check_window(self.shape, self.base)
        self.engine = engine
        import torch
        self.tsdf = torch.ones((self.nz, self.ny, self.nx), dtype=torch.float32, device=engine.device)
        self.weight = torch.zeros((self.nz, self.ny, self.nx), dtype=torch.float32, device=engine.device)
        self.n_scans = 0
        self.n_shifts = 0
        self.pieces = []                 # (T,3,3) float32 host arrays: what `follow` meshed and no `on_leave` took
        if store is not None and store is not False:
            from .tsdf_store import TsdfBrickStore
            self.store = TsdfBrickStore(engine) if store is True else store
            if not isinstance(self.store, TsdfBrickStore):
                raise ValueError("store must be None, True or a TsdfBrickStore, got %r" % (store,))
            self.store.bind(self)

    @property
    def shape(self) -> Tuple[int, int, int]:
        return self.nx, self.ny, self.nz

    @property
    def anchor(self) -> np.ndarray:
        return self.origin

    def _window(self) -> dict:
        return dict(base=self.base)

    def reset(self) -> None:
        """Back to the fresh window at the base it has; the pieces kept so far are dropped, and so is every brick of the store."""
        super().reset()
        self.pieces = []
        if self.store is not None:
            self.store.clear()

    def cell_of(self, position) -> Tuple[int, int, int]:
        """The lattice cell a point lies in: floor((position - anchor) / voxel) per axis."""
        p = np.asarray(position, np.float64).reshape(-1)
        if p.shape[0] != 3 or not np.isfinite(p).all():
            raise ValueError("position must be 3 finite numbers, got %r" % (position,))
        return tuple(int(v) for v in np.floor((p - self.origin) / self.voxel))

    def next_base(self, position) -> Tuple[int, int, int]:
        """The base `follow(position)` moves to: per axis, when the cell of `position` is `shift` voxels or more from the window's
        centre base + n // 2, the base moves by that distance rounded towards zero to a multiple of `shift`."""
        out = []
        for c, b, n in zip(self.cell_of(position), self.base, self.shape):
            d = c - (b + n // 2)
            out.append(b + (abs(d) // self.shift) * self.shift * (1 if d >= 0 else -1))
        return tuple(out)

    def follow(self, position, on_leave=None, min_weight: float = 1.0) -> bool:
        """Moves the window after the sensor at `position`; -> whether it moved.  Before the slots that change hands are cleared, the
        cells with at least one corner among the leaving samples are meshed -- at most three boxes of cells, `leaving_boxes` -- and
        every non-empty piece, an (T,3,3) float32 host array, goes to on_leave(piece), or into `self.pieces` without one.  With a
        store nothing is meshed (on_leave is refused): the leaving bricks are paged out, the window shifts, the entering bricks that
        the store holds are paged in.  A page-out over the store's max_bytes raises with window, base and store as they were."""
        if self.store is not None and on_leave is not None:
            raise ValueError("on_leave and store= exclude each other: with a store nothing is meshed when it leaves")
        new = self.next_base(position)
        if new == self.base:
            return False
        check_window(self.shape, new)
        if self.store is not None:
            self.store.page_out(self, leaving_boxes(self.base, new, self.shape))          # boxes of SAMPLES: the full shape
            self.engine.tsdf_window_shift(self.tsdf, self.weight, self.base, new)
            old, self.base = self.base, new
            self.store.page_in(self, leaving_boxes(new, old, self.shape))
            self.n_shifts += 1
            return True
        if self.n_scans > 0:                      # a window nothing was fused into has no surface to keep
            for lo, hi in leaving_boxes(self.base, new, tuple(n - 1 for n in self.shape)):      # boxes of CELLS, by their low corners
                tri = self.triangles(min_weight, box=(lo, hi))
                if int(tri.shape[0]) > 0:
                    piece = tri.cpu().numpy()
                    if on_leave is not None:
                        on_leave(piece)
                    else:
                        self.pieces.append(piece)
        self.engine.tsdf_window_shift(self.tsdf, self.weight, self.base, new)
        self.base = new
        self.n_shifts += 1
        return True

    def triangles(self, min_weight: float = 1.0, box=None):
        """(T,3,3) float32 device tensor, T >= 0: the triangles of the cells whose low corner lies in box = (lo, hi), hi exclusive, in
        ascending cell order within the box; box=None is every cell of the window.  A cell needs all eight corners in the window.
        With a store, box=None is every cell of window and store, once, in the order of the sweep's tiles
        (`TsdfBrickStore.triangles`)."""
        if np.isnan(float(min_weight)):
            raise ValueError("min_weight is NaN")
        if self.store is not None and box is None:
            return self.store.triangles(self, min_weight)
        top = tuple(b + n - 1 for b, n in zip(self.base, self.shape))
        lo, hi = (self.base, top) if box is None else (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
        if len(lo) != 3 or len(hi) != 3 or any(l > h or l < b or h > t for l, h, b, t in zip(lo, hi, self.base, top)):
            raise ValueError("the cells %s .. %s (exclusive) have corners outside the window %s .. %s" % (lo, hi, self.base, top))
        tri, total = self.engine.tsdf_triangles(self.tsdf, self.weight, self.origin, self.voxel, min_weight, base=self.base, box=(lo, hi))
        if total == 0:
            import torch
            return torch.zeros((0, 3, 3), dtype=torch.float32, device=self.engine.device)
        return tri

    def mesh(self, min_weight: float = 1.0) -> TriangleMesh:
        """The pieces kept by `follow` in the order they left, then the window, as one TriangleMesh (a soup).  With a store: the
        sweep of window and store (`triangles`), no cell twice."""
        parts = list(self.pieces) + [self.triangles(min_weight).cpu().numpy()]
        tri = np.concatenate(parts).astype(np.float32, copy=False)
        t = int(tri.shape[0])
        if t == 0:
            raise OvnError("RollingTsdfVolume.mesh: no surface: no cell has all eight corners seen %g times and a sign change "
                           "(%d scans fused)" % (min_weight, self.n_scans))
        if t > MAX_TRIANGLES:
            raise OvnError("RollingTsdfVolume.mesh: %d triangles exceed the 2^27 a TriangleMesh holds: use a larger voxel" % t)
        return TriangleMesh(np.ascontiguousarray(tri.reshape(3 * t, 3)), np.arange(3 * t, dtype=np.int32).reshape(t, 3))
