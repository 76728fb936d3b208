"""Overlap-based Monte Carlo localization in a map of keyframes (the second application of the network, after loop closing).

A map is M keyframes with known world poses (x, y, heading), cached in an `Infer`'s FeatureVolumeCache at slots 0 .. M - 1, and a
regular grid whose cells each name the keyframe nearest their centre (within `reach` metres) or nothing.  A particle is a pose
hypothesis (x, y, theta) with a weight.  One step of the filter:

  1. the query scan goes through the leg once (and through the spectrum of the yaw head);
  2. `ovn_mcl_predict`: odometry plus Philox noise moves every particle, each looks up the keyframe of its cell, and the distinct
     keyframes form an ascending list of U entries -- the host reads U from one 16-byte record;
  3. the 1-vs-U sweep over that list: overlap o_f and yaw y_f of every listed keyframe against the query;
  4. `ovn_mcl_update`: w *= max(o_f, o_min) * (eps + (1 - eps) exp(-d^2 / 2 sigma^2)), d = the particle's heading relative to the
     keyframe minus the network's yaw; weights rescaled by a power of two; the weighted mean pose and N_eff come back as 8 doubles;
  5. `ovn_mcl_resample` (systematic, exact in integers) when N_eff < resample_fraction * P.

The keyframes are recorded scans at known poses (`OverlapMap(...)`) or virtual scans rendered from a triangle mesh of the environment
at the poses of a grid (`OverlapMap.from_mesh`, `grid_poses`; csrc/render_mesh.hip): the filter does not care.

The kernels are csrc/mcl.hip; the formulas are stated in DESIGN.md, "Localization".  Everything but the two records and the estimate
stays on the device, and a step with the same seed and inputs gives the same bits.

The observation-model defaults (sigma_yaw, eps_yaw, overlap_min) are UNTUNED placeholders: no trained weights were at hand when this
was written.  Choose them on recorded data before relying on the filter.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import OvnError

MAX_PARTICLES = 65536        # OVN_MCL_MAX_PARTICLES of include/ovn_hip.h

Estimate = namedtuple("Estimate", "x y yaw n_eff resampled lost frames_scored off_map")


def poses_xyyaw(poses) -> np.ndarray:
    """(M,3) float64 rows x, y, heading [rad] from either such rows or (M,4,4) world poses (heading = atan2(R10, R00))."""
    a = np.asarray(poses, np.float64)
    if a.ndim == 3 and a.shape[1:] == (4, 4):
        return np.stack([a[:, 0, 3], a[:, 1, 3], np.arctan2(a[:, 1, 0], a[:, 0, 0])], axis=1)
    if a.ndim == 2 and a.shape[1] == 3:
        return a.copy()
    raise ValueError("poses must be (M,3) rows x, y, heading or (M,4,4) matrices, got %s" % (a.shape,))


def grid_for(xy: np.ndarray, resolution: float, reach: float):
    """(origin_x, origin_y, nx, ny) of the smallest grid, aligned to multiples of `resolution`, that holds every cell within
    `reach` of a keyframe."""
    res = float(resolution)
    lo = np.floor((xy.min(axis=0) - reach) / res)
    hi = np.floor((xy.max(axis=0) + reach) / res)
    nx, ny = int(hi[0] - lo[0]) + 1, int(hi[1] - lo[1]) + 1
    return float(lo[0] * res), float(lo[1] * res), nx, ny


def grid_poses(x_range, y_range, resolution: float, z: float, yaw: float = 0.0) -> np.ndarray:
    """(M,4,4) float64 sensor poses for `OverlapMap.from_mesh`: one per cell of the grid of `resolution` metres laid over
    [x_range[0], x_range[1]) x [y_range[0], y_range[1]), at the cell's centre, height `z`, heading `yaw` [rad]; rows run over y, then
    x (pose iy * nx + ix).  A range shorter than one cell still gives one cell."""
    res = float(resolution)
    if not res > 0:
        raise ValueError("resolution must be > 0")
    x0, x1 = float(x_range[0]), float(x_range[1])
    y0, y1 = float(y_range[0]), float(y_range[1])
    if not (x1 >= x0 and y1 >= y0):
        raise ValueError("ranges must be (low, high), got %s and %s" % (tuple(x_range), tuple(y_range)))
    nx = max(1, int(math.ceil((x1 - x0) / res - 1e-9)))
    ny = max(1, int(math.ceil((y1 - y0) / res - 1e-9)))
    cx = x0 + (np.arange(nx) + 0.5) * res
    cy = y0 + (np.arange(ny) + 0.5) * res
    poses = np.zeros((ny, nx, 4, 4), np.float64)
    c, s = math.cos(float(yaw)), math.sin(float(yaw))
    poses[:, :] = np.array([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, float(z)], [0.0, 0.0, 0.0, 1.0]])
    poses[:, :, 0, 3] = cx[None, :]
    poses[:, :, 1, 3] = cy[:, None]
    return poses.reshape(ny * nx, 4, 4)


def keep_scans(valid_pixels, n_pixels: int, min_valid_fraction: float) -> np.ndarray:
    """The drop rule of `OverlapMap.from_mesh`: a rendered scan with fewer than min_valid_fraction * n_pixels valid pixels is dropped
    (the pose sits inside a wall or off the mesh).  Returns the boolean keep mask of the per-scan counts."""
    return np.asarray(valid_pixels, np.float64) >= float(min_valid_fraction) * float(n_pixels)


def render_chunk(h: int, w: int, c: int, budget_bytes: int = 1 << 28) -> int:
    """Poses `from_mesh` renders per pass: the range image and the stacked leg input of a chunk take at most `budget_bytes` (256 MB)
    beside the leg's workspace, and a chunk is at most the 1024 scans the leg processes per pass."""
    return int(max(1, min(1024, budget_bytes // (4 * h * w * (c + 1)))))


def build_cell_frame(xy, origin_x: float, origin_y: float, resolution: float, nx: int, ny: int, reach: Optional[float] = None) -> np.ndarray:
    """The int32 table cell_frame[iy * nx + ix]: the keyframe nearest the cell's centre among those within `reach` metres of it
    (default: `resolution`), -1 where there is none; equal distances go to the smaller frame id.  NumPy only, one window per frame."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    res = float(resolution)
    reach = res if reach is None else float(reach)
    if not res > 0 or not reach > 0:
        raise ValueError("resolution and reach must be > 0")
    if nx < 1 or ny < 1 or nx * ny > 2 ** 31 - 1:
        raise ValueError("grid %d x %d outside 1 .. 2^31 - 1 cells" % (nx, ny))
    best = np.full((ny, nx), np.inf)
    table = np.full((ny, nx), -1, np.int32)
    for f, (x, y) in enumerate(xy):
        ix0 = max(int(math.floor((x - reach - origin_x) / res - 0.5)), 0)
        ix1 = min(int(math.ceil((x + reach - origin_x) / res - 0.5)), nx - 1)
        iy0 = max(int(math.floor((y - reach - origin_y) / res - 0.5)), 0)
        iy1 = min(int(math.ceil((y + reach - origin_y) / res - 0.5)), ny - 1)
        if ix0 > ix1 or iy0 > iy1:
            continue
        cx = origin_x + (np.arange(ix0, ix1 + 1) + 0.5) * res
        cy = origin_y + (np.arange(iy0, iy1 + 1) + 0.5) * res
        d2 = (cy[:, None] - y) ** 2 + (cx[None, :] - x) ** 2
        win_best, win_tab = best[iy0:iy1 + 1, ix0:ix1 + 1], table[iy0:iy1 + 1, ix0:ix1 + 1]
        take = (d2 <= reach * reach) & (d2 < win_best)
        win_best[take] = d2[take]
        win_tab[take] = f
    return table.reshape(-1)


def cell_of(x, y, origin_x: float, origin_y: float, resolution: float, nx: int, ny: int) -> np.ndarray:
    """The lookup of `ovn_mcl_predict` restated in NumPy float32, operation for operation: the cell index iy * nx + ix of every
    position, -1 outside the grid or for a non-finite coordinate."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    inv = np.float32(1.0 / float(resolution))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((x - np.float32(origin_x)) * inv)
        fy = np.floor((y - np.float32(origin_y)) * inv)
        ok = (fx >= 0) & (fx < np.float32(2147483648.0)) & (fy >= 0) & (fy < np.float32(2147483648.0))
        ix = np.where(ok, fx, 0).astype(np.int64)
        iy = np.where(ok, fy, 0).astype(np.int64)
    ok &= (ix < nx) & (iy < ny)
    return np.where(ok, iy * nx + ix, -1)


def _features_of(infer, scan) -> torch.Tensor:
    """One scan through the leg -> (1, W, 128) on the device.  `scan`: a frame name of the Infer's data set (str or int, read as
    `Infer` reads a current frame), an (N,4) float32 point cloud (projected on the GPU with the Infer's input flags), or a
    (1,H,W,C) / (H,W,C) leg input tensor."""
    eng = infer.engine
    if isinstance(scan, torch.Tensor):
        x = scan if scan.dim() == 4 else scan.unsqueeze(0)
        return eng.leg(x.to(eng.device, torch.float32).contiguous())
    if isinstance(scan, np.ndarray):
        if infer.use_class_probabilities:
            raise OvnError("a raw point cloud carries no class probabilities: pass a frame name")
        from .preprocess import project_scans
        h, w = int(infer.inputShape[0]), int(infer.inputShape[1])
        r = project_scans([scan], engine=eng, proj_H=h, proj_W=w, want=(),
                          stacked_flags=(bool(infer.use_depth), bool(infer.use_normals), bool(infer.use_intensity)))
        return eng.leg(r["stacked"])
    name = str(scan).zfill(6) if isinstance(scan, (int, np.integer)) else str(scan)
    return infer._leg_device([name])


class OverlapMap(object):
    """M keyframes with poses, cached through `infer`, plus the grid that sends a position to its keyframe."""

    def __init__(self, infer, frame_names: Optional[Sequence], poses, resolution: float, reach: Optional[float] = None, scans=None):
        """frame_names: the keyframes as `Infer` names frames (read from its data set), or None with `scans`, a list of (N,4) clouds.
        poses: (M,3) rows x, y, heading [rad] or (M,4,4) world poses.  The Infer's cache must be empty: the map takes slots 0 .. M-1."""
        if getattr(infer, "_world", 1) > 1:
            raise OvnError("OverlapMap: a sharded Infer (world %d) is not supported: the sweep of a localization step runs on one GPU; "
                           "build the map on a single-rank Infer" % infer._world)
        self.infer = infer
        self.engine = infer.engine
        self.poses = poses_xyyaw(poses)
        m = self.poses.shape[0]
        items = list(scans) if scans is not None else list(frame_names or [])
        if m < 1 or len(items) != m:
            raise ValueError("OverlapMap: %d poses for %d keyframes" % (m, len(items)))
        if len(infer.feature_volumes) != 0:
            raise OvnError("OverlapMap: the Infer already caches %d frames; the map needs slots 0 .. M-1 (infer.feature_volumes = [])"
                           % len(infer.feature_volumes))
        self.frame_names = [str(n) for n in frame_names] if frame_names is not None else [str(i) for i in range(m)]
        self.resolution = float(resolution)
        self.reach = self.resolution if reach is None else float(reach)
        self.origin_x, self.origin_y, self.nx, self.ny = grid_for(self.poses[:, :2], self.resolution, self.reach)
        self.cell_frame_host = build_cell_frame(self.poses[:, :2], self.origin_x, self.origin_y, self.resolution, self.nx, self.ny,
                                                self.reach)
        bs = max(1, int(infer.batch_size))
        cache = infer.feature_volumes
        if scans is not None:
            for s in items:
                cache.extend_device(_features_of(infer, np.asarray(s, np.float32)))
        else:
            names = [str(n).zfill(6) if isinstance(n, (int, np.integer)) else str(n) for n in items]
            for a in range(0, m, bs):
                cache.extend_device(infer._leg_device(names[a:a + bs]))
        dev = self.engine.device
        self.cell_frame = torch.from_numpy(self.cell_frame_host).to(dev)
        self.frame_yaw = torch.from_numpy(self.poses[:, 2].astype(np.float32)).to(dev)

    @property
    def n_frames(self) -> int:
        return self.poses.shape[0]

    @property
    def occupied_cells(self) -> np.ndarray:
        """Indices iy * nx + ix of the cells that name a keyframe, ascending."""
        return np.nonzero(self.cell_frame_host >= 0)[0]

    def cell_centre(self, cells) -> np.ndarray:
        cells = np.asarray(cells, np.int64)
        return np.stack([self.origin_x + (cells % self.nx + 0.5) * self.resolution,
                         self.origin_y + (cells // self.nx + 0.5) * self.resolution], axis=-1)

    kept = None             # from_mesh: indices into the poses it was given of the map frames it kept (None for a keyframe map)
    mesh_built = False

    @classmethod
    def from_mesh(cls, infer, mesh, poses, resolution: float, reach: Optional[float] = None, min_valid_fraction: float = 0.1,
                  chunk: Optional[int] = None, fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0,
                  min_range: float = 0.0) -> "OverlapMap":
        """A map whose frames are virtual scans of `mesh` (mesh.TriangleMesh) rendered at `poses`, (M,4,4) sensor poses in the mesh's
        frame (`grid_poses` makes one per grid cell): the map of Chen et al., which has a frame wherever the robot can be.  The scans
        are rendered `chunk` poses at a time (default: `render_chunk`), each chunk goes through the leg into the Infer's cache.  A
        pose whose scan has fewer than min_valid_fraction * H * W valid pixels (inside a wall, off the mesh) is dropped before the
        cell table is built; `map.kept` lists the indices of the others.  The sensor (fov_up, fov_down, max_range) defaults to the
        one `MonteCarloLocalizer.step` projects a raw query cloud with.  min_range: a pixel counts as valid for the drop rule when
        its range exceeds it -- the blind zone of a real sensor.  The mesh is two-sided, so a pose inside a closed solid sees that
        solid from inside in every pixel and the default 0 keeps it; with min_range above the solid's half width it is dropped.  The
        rendered images themselves are not changed by it."""
        def render(eng, p, h, w, flags):
            return eng.render_scans(mesh, p, h, w, fov_up, fov_down, max_range, want=("range",), stacked_flags=flags)
        return cls._from_renderer("OverlapMap.from_mesh", "the mesh's", render, infer, poses, resolution, reach, min_valid_fraction,
                                  chunk, fov_up, fov_down, max_range, min_range)

    @classmethod
    def from_tsdf(cls, infer, volume, poses, resolution: float, reach: Optional[float] = None, min_valid_fraction: float = 0.1,
                  chunk: Optional[int] = None, fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0,
                  min_range: float = 0.0, ray_min_range: float = 0.5, step: Optional[float] = None,
                  min_weight: float = 1.0) -> "OverlapMap":
        """`from_mesh` without the mesh: the map's frames are views of `volume` (tsdf.TsdfVolume) ray-cast at `poses`
        (`TsdfVolume.render_scans`, ovn_tsdf_raycast).  Chunking, the keep rule (min_valid_fraction, min_range) and the caching are
        those of `from_mesh`; ray_min_range, step and min_weight are the march parameters of the ray caster.  The brick mask is built
        once for the whole map.  A map built this way is saved and loaded as a mesh-built one is, with the volume's `mesh()` or the
        volume re-fused by the caller; `load` itself renders from a mesh."""
        mask = []                        # built by the first chunk: the shared part checks its arguments before any GPU work

        def render(eng, p, h, w, flags):
            if eng is not volume.engine:
                raise OvnError("OverlapMap.from_tsdf: the volume lives on another engine than the Infer's")
            if not mask:
                mask.append(volume.bricks(min_weight))
            return volume.render_scans(p, h, w, fov_up, fov_down, ray_min_range, max_range, step, min_weight, bricks=mask[0],
                                       want=("range",), stacked_flags=flags)
        return cls._from_renderer("OverlapMap.from_tsdf", "the volume's", render, infer, poses, resolution, reach, min_valid_fraction,
                                  chunk, fov_up, fov_down, max_range, min_range)

    @classmethod
    def _from_renderer(cls, what, whose, render, infer, poses, resolution, reach, min_valid_fraction, chunk, fov_up, fov_down,
                       max_range, min_range) -> "OverlapMap":
        """The part `from_mesh` and `from_tsdf` share: render(engine, poses, H, W, flags) -> dict(range, stacked) per chunk, the keep
        rule, the leg, the cache and the cell table."""
        if getattr(infer, "_world", 1) > 1:
            raise OvnError("%s: a sharded Infer (world %d) is not supported: build the map on a single-rank Infer"
                           % (what, infer._world))
        if infer.use_intensity or infer.use_class_probabilities:
            raise OvnError("%s: a rendered scan has no intensity and no class probabilities, but this Infer's model "
                           "takes %s; use a model with depth and / or normals only"
                           % (what, " and ".join(n for n, f in (("intensity", infer.use_intensity),
                                                                ("class probabilities", infer.use_class_probabilities)) if f)))
        if len(infer.feature_volumes) != 0:
            raise OvnError("%s: the Infer already caches %d frames; the map needs slots 0 .. M-1 "
                           "(infer.feature_volumes = [])" % (what, len(infer.feature_volumes)))
        p = np.ascontiguousarray(np.asarray(poses, np.float64))
        if p.ndim != 3 or p.shape[1:] != (4, 4) or p.shape[0] < 1:
            raise ValueError("%s: poses must be (M,4,4) with M >= 1, got %s" % (what, p.shape))
        eng = infer.engine
        h, w, c = (int(v) for v in infer.inputShape)
        step = render_chunk(h, w, c) if chunk is None else max(1, int(chunk))
        flags = (bool(infer.use_depth), bool(infer.use_normals))
        cache = infer.feature_volumes
        keep = np.zeros(p.shape[0], bool)
        for a in range(0, p.shape[0], step):
            r = render(eng, p[a:a + step], h, w, flags)
            k = keep_scans((r["range"] > float(min_range)).sum(dim=(1, 2)).cpu().numpy(), h * w, min_valid_fraction)
            keep[a:a + step] = k
            if k.all():
                cache.extend_device(eng.leg(r["stacked"]))
            elif k.any():
                cache.extend_device(eng.leg(r["stacked"][torch.from_numpy(np.nonzero(k)[0]).to(eng.device)].contiguous()))
        kept = np.nonzero(keep)[0]
        if len(kept) == 0:
            raise OvnError("%s: none of the %d poses sees %g of its pixels: are they in %s frame?"
                           % (what, p.shape[0], min_valid_fraction, whose))
        self = cls.__new__(cls)
        self.infer, self.engine = infer, eng
        self.mesh_built, self.kept, self.sensor_poses = True, kept, p[kept]
        self.min_valid_fraction, self.sensor = float(min_valid_fraction), (float(fov_up), float(fov_down), float(max_range))
        self.min_range = float(min_range)
        self.poses = poses_xyyaw(self.sensor_poses)
        self.frame_names = ["mesh:%d" % i for i in kept]
        self.resolution = float(resolution)
        self.reach = self.resolution if reach is None else float(reach)
        self.origin_x, self.origin_y, self.nx, self.ny = grid_for(self.poses[:, :2], self.resolution, self.reach)
        self.cell_frame_host = build_cell_frame(self.poses[:, :2], self.origin_x, self.origin_y, self.resolution, self.nx, self.ny,
                                                self.reach)
        self.cell_frame = torch.from_numpy(self.cell_frame_host).to(eng.device)
        self.frame_yaw = torch.from_numpy(self.poses[:, 2].astype(np.float32)).to(eng.device)
        return self

    def save(self, path: str) -> None:
        """What rebuilds the map: names, poses, resolution, reach (the feature volumes are recomputed through the leg by `load`).  A
        mesh-built map adds its marker, the kept sensor poses, their indices, the drop threshold and the sensor; the mesh is the
        caller's to keep."""
        if self.mesh_built:
            np.savez(path, frame_names=np.asarray(self.frame_names), poses=self.poses, resolution=self.resolution, reach=self.reach,
                     mesh_built=np.int32(1), sensor_poses=self.sensor_poses, kept=self.kept.astype(np.int64),
                     min_valid_fraction=self.min_valid_fraction, sensor=np.asarray(self.sensor, np.float64),
                     min_range=self.min_range)
            return
        np.savez(path, frame_names=np.asarray(self.frame_names), poses=self.poses, resolution=self.resolution, reach=self.reach)

    @classmethod
    def load(cls, infer, path: str, mesh=None) -> "OverlapMap":
        """`mesh`: the TriangleMesh of a mesh-built map (its scans are rendered again); a keyframe map takes none."""
        with np.load(path) as z:
            if "mesh_built" in z.files:
                if mesh is None:
                    raise OvnError("OverlapMap.load: %s holds a mesh-built map: pass the mesh (load(infer, path, mesh))" % path)
                up, down, rmax = (float(v) for v in z["sensor"])
                m = cls.from_mesh(infer, mesh, z["sensor_poses"], float(z["resolution"]), float(z["reach"]),
                                  float(z["min_valid_fraction"]), fov_up=up, fov_down=down, max_range=rmax,
                                  min_range=float(z["min_range"]))
                if len(m.kept) != len(z["kept"]):
                    raise OvnError("OverlapMap.load: %d of the %d saved map frames see too little of this mesh: not the mesh the map "
                                   "was built from" % (len(z["kept"]) - len(m.kept), len(z["kept"])))
                m.kept = z["kept"].astype(np.int64)
                m.frame_names = [str(n) for n in z["frame_names"]]
                return m
            if mesh is not None:
                raise OvnError("OverlapMap.load: %s holds a keyframe map, which takes no mesh" % path)
            return cls(infer, [str(n) for n in z["frame_names"]], z["poses"], float(z["resolution"]), float(z["reach"]))


class MonteCarloLocalizer(object):
    """The particle filter.  sigma_yaw [deg], eps_yaw and overlap_min shape the observation model (module docstring: untuned
    defaults).  resample_fraction: resample when N_eff < fraction * P.  converged_particles / converge_radius: once the weighted rms
    distance of the particles from their mean is under `converge_radius` metres, a resample goes down to `converged_particles`.
    `lost` (no particle on the map, or no positive weight) re-runs `init_uniform` with the full count."""

    def __init__(self, map: OverlapMap, n_particles: int, seed: int = 0, sigma_yaw: float = 10.0, eps_yaw: float = 0.1,
                 overlap_min: float = 0.01, resample_fraction: float = 0.5, converged_particles: Optional[int] = None,
                 converge_radius: float = 1.0):
        n = int(n_particles)
        if not 1 <= n <= MAX_PARTICLES:
            raise ValueError("n_particles must be in 1..%d, got %d" % (MAX_PARTICLES, n))
        if converged_particles is not None and not 1 <= int(converged_particles) <= n:
            raise ValueError("converged_particles must be in 1..n_particles")
        if not sigma_yaw > 0 or not overlap_min > 0 or not 0 <= eps_yaw <= 1:
            raise ValueError("sigma_yaw and overlap_min must be > 0, eps_yaw in [0, 1]")
        self.map, self.engine = map, map.engine
        self.n_particles, self.seed = n, int(seed)
        self.sigma_yaw, self.eps_yaw, self.overlap_min = float(sigma_yaw), float(eps_yaw), float(overlap_min)
        self.resample_fraction = float(resample_fraction)
        self.converged_particles = None if converged_particles is None else int(converged_particles)
        self.converge_radius = float(converge_radius)
        dev = self.engine.device
        self._buf = [torch.zeros((n, 4), dtype=torch.float32, device=dev) for _ in range(2)]
        self._cur, self._p = 0, n
        m = map.n_frames
        self._pframe = torch.empty(n, dtype=torch.int32, device=dev)
        self._slot = torch.empty(m, dtype=torch.int32, device=dev)
        self._list = torch.empty(m, dtype=torch.int32, device=dev)
        self._anc = torch.empty(n, dtype=torch.int32, device=dev)
        self._est = torch.empty(8, dtype=torch.float64, device=dev)
        self._rec = torch.zeros((2, 4), dtype=torch.int32).pin_memory()       # predict's and resample's 16-byte records
        self._rec_np = self._rec.numpy()
        self._step = 0
        self._inits = 0
        self.last = {}           # device tensors of the last step, for inspection: overlap, yaw, frame_list, ancestors
        self.init_uniform()

    @property
    def particles(self) -> torch.Tensor:
        """The current (P,4) float32 device tensor of rows x, y, theta, w."""
        return self._buf[self._cur][:self._p]

    def _upload(self, rows: np.ndarray) -> None:
        self._cur, self._p = 0, rows.shape[0]
        self._buf[0][:self._p].copy_(torch.from_numpy(np.ascontiguousarray(rows, np.float32)))

    def init_uniform(self) -> None:
        """n_particles spread over the occupied cells: cell, position inside it and heading from a NumPy generator seeded by
        (seed, number of initialisations so far); weights 1."""
        g = np.random.default_rng([self.seed, self._inits])
        self._inits += 1
        cells = self.map.occupied_cells
        if len(cells) == 0:
            raise OvnError("the map has no occupied cell")
        c = cells[g.integers(0, len(cells), self.n_particles)]
        res = self.map.resolution
        rows = np.empty((self.n_particles, 4), np.float64)
        rows[:, 0] = self.map.origin_x + (c % self.map.nx + g.uniform(0.0, 1.0, self.n_particles)) * res
        rows[:, 1] = self.map.origin_y + (c // self.map.nx + g.uniform(0.0, 1.0, self.n_particles)) * res
        rows[:, 2] = -g.uniform(-math.pi, math.pi, self.n_particles)        # (-pi, pi]
        rows[:, 3] = 1.0
        self._upload(rows)

    def init_around(self, pose, sigma) -> None:
        """n_particles drawn around pose = (x, y, theta) with standard deviations sigma = (sx, sy, stheta); weights 1."""
        g = np.random.default_rng([self.seed, self._inits])
        self._inits += 1
        rows = np.empty((self.n_particles, 4), np.float64)
        for k in range(3):
            rows[:, k] = float(pose[k]) + float(sigma[k]) * g.standard_normal(self.n_particles)
        rows[:, 2] = -((-rows[:, 2] + math.pi) % (2.0 * math.pi) - math.pi)  # (-pi, pi]
        rows[:, 3] = 1.0
        self._upload(rows)

    def step(self, scan, odom, sigma) -> Estimate:
        """One localization step: `scan` as `_features_of` takes it, odom = (dx, dy, dtheta) in the robot frame since the last step,
        sigma = (sigma_x, sigma_y, sigma_theta) of its noise."""
        mp, eng = self.map, self.engine
        cache = mp.infer.feature_volumes
        m = mp.n_frames
        if len(cache) < m:
            raise OvnError("the Infer's cache no longer holds the map (%d of %d frames)" % (len(cache), m))
        q = _features_of(mp.infer, scan)
        spec = eng.spectrum(q) if cache.spectral else None
        step = self._step
        self._step += 1
        stream = torch.cuda.current_stream(eng.device)
        parts = self.particles
        eng.mcl_predict(parts, odom, sigma, self.seed, step, mp.cell_frame, (mp.origin_x, mp.origin_y), mp.resolution, mp.nx, mp.ny, m,
                        particle_frame=self._pframe[:self._p], frame_slot=self._slot, frame_list=self._list, record=self._rec[0])
        stream.synchronize()
        u, off_map = int(self._rec_np[0, 0]), int(self._rec_np[0, 1])
        overlap = yaw = None
        if u > 0:
            feats = cache.device_features[:m]
            dc = cache.device_delta_cache
            r = eng.heads(feats, q, lidx=self._list[:u], n=u, spec_l=None if spec is None else cache.device_spectra[:m], spec_r=spec,
                          dcache_l=None if (dc is None or spec is None) else dc[:m])
            overlap, yaw = r["overlap"], r["yaw"]
        want_spread = self.converged_particles is not None
        res = eng.mcl_update(parts, self._pframe[:self._p], self._slot, mp.frame_yaw, overlap, yaw, self.sigma_yaw, self.eps_yaw,
                             self.overlap_min, estimate=self._est, want_spread=want_spread)
        if want_spread:
            e = torch.cat([res[0], res[1]]).cpu().numpy()
        else:
            e = res.cpu().numpy()
        self.last = {"overlap": overlap, "yaw": yaw, "frame_list": self._list[:u], "estimate": e[:8].copy()}
        lost = e[0] != 0 or off_map == self._p
        resampled = False
        if not lost and e[2] < self.resample_fraction * self._p:
            n_out = self._p
            if want_spread and e[8] < self.converge_radius:
                n_out = min(self._p, self.converged_particles)
            nxt = self._cur ^ 1
            eng.mcl_resample(parts, self.seed, step, n_out=n_out, out=self._buf[nxt][:n_out], ancestors=self._anc[:n_out],
                             record=self._rec[1])
            stream.synchronize()
            if int(self._rec_np[1, 0]) != 0:
                lost = True
            else:
                self._cur, self._p, resampled = nxt, n_out, True
                self.last["ancestors"] = self._anc[:n_out]
        if lost:
            self.init_uniform()
        return Estimate(float(e[3]), float(e[4]), float(e[5]), float(e[2]), resampled, bool(lost), u, off_map)
