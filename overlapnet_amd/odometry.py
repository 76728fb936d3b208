"""LiDAR odometry: the poses every mapping step of this package asks for, from the scans alone.

    poses, regs = frame_to_frame(engine, points, offsets)             # scan i + 1 registered onto scan i, chained
    odo = TsdfOdometry(engine, lo, hi, voxel=0.2)                     # frame to MODEL: predict, ray-cast, register, fuse
    for scan in scans: result = odo.track(scan)
    poses, results, volume = estimate_poses(engine, points, offsets)  # both in a row; `volume.mesh()` is the map's mesh
    odo = RollingTsdfOdometry(engine, extent=(120, 120, 20), voxel=0.2)   # the same tracker in a window that follows the sensor (section 36)
    poses, results, volume = estimate_poses(engine, points, offsets, window=120.0)    # online: no first pass, any drive length
    odo = TsdfOdometry(engine, lo, hi, voxel=0.2, deskew=dict(t_ref=0.5)); odo.track(scan, times=fractions)   # raw sweeps (section 37)

The pieces are HIP kernels that exist on their own: `ovn_project` (range, vertex and normal images), `ovn_tsdf_raycast` (the model seen
from the predicted pose), `ovn_icp_register` (the alignment of two such images) and `ovn_tsdf_integrate` (the model).  This module is
the plumbing between them.  Poses are sensor-to-world 4 x 4 matrices; the first one is the identity unless the caller says otherwise.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

SOURCE_FIRST, SOURCE_MODEL, SOURCE_FRAME, SOURCE_PREDICTION = "first", "model", "frame", "prediction"
_SOURCES = (SOURCE_MODEL, SOURCE_FRAME, SOURCE_PREDICTION)


class TrackResult(NamedTuple):
    pose: np.ndarray          # (4,4) f64 sensor to world
    source: str               # "first", "model", "frame" (registered onto the previous scan) or "prediction" (nothing registered)
    status: int               # the status of the registration that gave the pose (0 ok); of the frame registration for "prediction"
    fitness: float            # inliers / valid source pixels of that registration
    rms: float
    inliers: int


def bounds_from_poses(poses, max_range: float, below: float = 5.0, above: float = 15.0) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi): the sensor positions' bounding box grown by max_range in x and y, by `below` / `above` metres in z."""
    o = np.asarray(poses, np.float64)[:, :3, 3]
    lo, hi = o.min(axis=0), o.max(axis=0)
    return (np.array([lo[0] - max_range, lo[1] - max_range, lo[2] - below]),
            np.array([hi[0] + max_range, hi[1] + max_range, hi[2] + above]))


def predict(t_prev: np.ndarray, t_last: np.ndarray) -> np.ndarray:
    """Constant velocity: the last step, T_prev^-1 T_last, taken once more from T_last."""
    t_prev, t_last = np.asarray(t_prev, np.float64), np.asarray(t_last, np.float64)
    return t_last @ (np.linalg.inv(t_prev) @ t_last)


def write_poses(path: str, poses) -> None:
    """KITTI pose lines: the 12 numbers of the upper 3 x 4 of every pose, one pose per line, written so that they read back to the
    same float64 values (`tools/build_mesh.py --poses` without --calib takes the file)."""
    p = np.asarray(poses, np.float64)
    if p.ndim != 3 or p.shape[1:] != (4, 4):
        raise ValueError("poses must be (n,4,4), got %s" % (p.shape,))
    with open(path, "w") as f:
        for m in p:
            f.write(" ".join(repr(float(x)) for x in m[:3].reshape(-1)) + "\n")


def _check_scans(points, offsets) -> np.ndarray:
    offs = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets, np.int64).reshape(-1)
    shape = tuple(points.shape)
    if len(shape) != 2 or shape[1] != 4:
        raise ValueError("points must be (total,4), got %s" % (shape,))
    if offs.shape[0] < 1 or offs[0] < 0 or np.any(np.diff(offs) < 0) or offs[-1] > shape[0]:
        raise ValueError("offsets must ascend within the %d points" % shape[0])
    return offs


def frame_to_frame(engine, points, offsets, proj_h: int = 64, proj_w: int = 900, fov_up: float = 3.0, fov_down: float = -25.0,
                   max_range: float = 50.0, chunk: int = 64, first_pose=None, **icp_params):
    """Scan i + 1 registered onto scan i from the identity for every i, `chunk` pairs per projection and `icp_register` launch, and
    the steps chained: T_0 = first_pose (the identity), T_{i+1} = T_i D_i.  A pair whose registration ends with status != 0 repeats the
    step before it (the identity for pair 0); its Registration carries that status.  points (total,4) float32 of concatenated scans,
    offsets (n+1) int64.  -> (poses (n,4,4) f64, [Registration] * (n - 1))."""
    import torch
    from .registration import decode_registrations
    offs = _check_scans(points, offsets)
    if int(chunk) < 1 or int(proj_h) < 1 or int(proj_w) < 1:
        raise ValueError("chunk, proj_h and proj_w must be >= 1, got %r, %r, %r" % (chunk, proj_h, proj_w))
    n = offs.shape[0] - 1
    t0 = np.eye(4) if first_pose is None else np.asarray(first_pose, np.float64).reshape(4, 4)
    if n <= 0:
        return np.zeros((0, 4, 4)), []
    dev = engine.device
    pts = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, np.float32))
    pts = pts.to(dev, torch.float32).contiguous()
    d_offs = torch.from_numpy(offs).to(dev)
    regs = []
    for a in range(0, n - 1, int(chunk)):                    # pairs a .. b - 1 need scans a .. b
        b = min(n - 1, a + int(chunk))
        m = engine.project(pts, d_offs[a:b + 2], max(int(np.diff(offs[a:b + 2]).max()), 1), int(proj_h), int(proj_w), fov_up, fov_down,
                           max_range, want=("range", "vertex", "normal"))
        k = b - a
        src = torch.arange(1, k + 1, dtype=torch.int32, device=dev)
        tgt = torch.arange(0, k, dtype=torch.int32, device=dev)
        init = torch.eye(4, dtype=torch.float64, device=dev).repeat(k, 1, 1)
        pose, stats = engine.icp_register(m["vertex"], m["normal"], m["range"], src, tgt, init, fov_up=fov_up, fov_down=fov_down,
                                          max_range=max_range, **icp_params)
        regs += decode_registrations(pose, stats)
    poses = np.empty((n, 4, 4))
    poses[0] = t0
    step = np.eye(4)
    for i, r in enumerate(regs):
        if r.status == 0:
            step = r.pose
        poses[i + 1] = poses[i] @ step
    return poses, regs


class TsdfOdometry(object):
    """Frame-to-model tracking against a TSDF volume over the box lo .. hi that grows with every tracked scan.

    track(points) per scan: predict the pose (constant velocity), project the scan, ray-cast the volume at the prediction, register
    the scan onto that view from the identity, pose = prediction . registration, fuse the scan at its pose.  If the registration onto
    the model ends with status != 0 (or below `min_fitness` when one is given) the scan's registration onto the PREVIOUS scan decides
    (source "frame"); if that fails too the prediction stands (source "prediction") and the scan is not fused.  No default
    `min_fitness` is chosen here: none has been measured.  **icp_params: iterations, max_dist, cos_min, huber, min_inliers.

    The device buffers hold three images each: slot 0 the virtual scan, slot 1 the current scan, slot 2 the previous scan.  Both
    registrations of a frame run in one launch, the choice between them is made on the device, and a frame reads back one pose and one
    stats row.  use_bricks=True rebuilds the brick mask of `ovn_tsdf_bricks` before every view; for the single view of a frame that
    costs more than it saves, so it is off by default.

    deskew: None (the default) takes every scan as a snapshot and makes the launches it always made.  A dict
    (`deskew.check_config`: t_ref, and start_azimuth with clockwise when the scans come without per-point times) takes the scans as RAW
    sweeps: scan k >= 2 is moved into the sensor frame of fraction t_ref of its sweep (`deskew.deskew_scans`) before it is projected,
    under the twist xi = Log(T_{k-2}^-1 T_{k-1}), the step `predict` repeats.  Scans 0 and 1 have no motion estimate when they are
    registered: they are registered and fused as they come.  When scan 2 arrives the first step is known, and before anything else the
    model is rebuilt from scans 0 and 1 deskewed by it (the volume is reset and the two are fused again at their poses; their raw
    points stay on the device until then).  Without that the model keeps a bent seed, and a deskewed scan registered onto a bent model
    comes out WORSE than a bent scan on a bent model, which at least share their distortion (measured: DESIGN.md section 37).  The
    pose of a scan is the sensor's pose at fraction t_ref of its sweep.  deskew_passes=2 deskews scan k >= 1 once more before it is
    FUSED, by the step Log(T_{k-1}^-1 T_k) its registration just found, and projects it again; there is no second registration.  The
    step comes from the pose the frame's one read-back brought (the read-back precedes the fusion), so a frame still reads back once;
    the twist travels host to device."""

    def __init__(self, engine, lo, hi, voxel: float, trunc: Optional[float] = None, proj_h: int = 64, proj_w: int = 900,
                 fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0, min_range: float = 0.5,
                 min_fitness: Optional[float] = None, max_weight: float = 64.0, min_weight: float = 1.0, use_bricks: bool = False,
                 deskew: Optional[dict] = None, deskew_passes: int = 1, **icp_params):
        from .tsdf import TsdfVolume, check_march
        if int(proj_h) < 1 or int(proj_w) < 1:
            raise ValueError("proj_h and proj_w must be >= 1, got %r, %r" % (proj_h, proj_w))
        check_march(min_range, max_range, voxel)
        if min_fitness is not None and not 0.0 <= float(min_fitness) <= 1.0:
            raise ValueError("min_fitness must lie in 0 .. 1, got %r" % (min_fitness,))
        bad = [k for k in icp_params if k not in ("iterations", "max_dist", "cos_min", "huber", "min_inliers")]
        if bad:
            raise ValueError("unknown registration parameters %s" % bad)
        from .deskew import check_config
        self.deskew = check_config(deskew)
        if deskew_passes not in (1, 2):
            raise ValueError("deskew_passes must be 1 or 2, got %r" % (deskew_passes,))
        self.deskew_passes = int(deskew_passes)
        self._seed: list = []                     # with deskew: (raw scan, times) of scans 0 and 1 on the device, until scan 2 arrives
        self.volume = self._make_volume(engine, lo, hi, voxel, trunc, max_weight, float(max_range))   # refuses bad bounds before the GPU
        import torch
        self.engine = engine
        self.h, self.w = int(proj_h), int(proj_w)
        self.sensor = (float(fov_up), float(fov_down), float(max_range))
        self.min_range, self.min_weight = float(min_range), float(min_weight)
        self.min_fitness = None if min_fitness is None else float(min_fitness)
        self.use_bricks = bool(use_bricks)
        self.icp_params = dict(icp_params)
        dev = engine.device
        self.range = torch.full((3, self.h, self.w), -1.0, dtype=torch.float32, device=dev)
        self.vertex = torch.full((3, self.h, self.w, 4), -1.0, dtype=torch.float32, device=dev)
        self.normal = torch.full((3, self.h, self.w, 3), -1.0, dtype=torch.float32, device=dev)
        self._src = torch.tensor([1, 1], dtype=torch.int32, device=dev)
        self._tgt = torch.tensor([0, 2], dtype=torch.int32, device=dev)
        self._init = torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1)
        self._offs = torch.zeros(2, dtype=torch.int64, device=dev)
        self.poses: List[np.ndarray] = []
        self.results: List[TrackResult] = []

    def _make_volume(self, engine, lo, hi, voxel, trunc, max_weight, max_range):
        from .tsdf import TsdfVolume
        return TsdfVolume(engine, lo, hi, voxel, trunc=trunc, max_weight=max_weight)

    def _before_view(self, pose: np.ndarray) -> None:
        """Called with the pose a scan is expected at (the first pose, then every prediction) before the volume is read or written."""

    def _project(self, points) -> None:
        """The scan's images into slot 1 (an empty scan: every pixel empty, without a launch)."""
        import torch
        n = int(points.shape[0])
        if n == 0:
            for t in (self.range, self.vertex, self.normal):
                t[1].fill_(-1.0)
            return
        dev = self.engine.device
        pts = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, np.float32))
        pts = pts.to(dev, torch.float32).contiguous()
        self._offs[1] = n
        up, down, rmax = self.sensor
        m = self.engine.project(pts, self._offs, n, self.h, self.w, up, down, rmax, want=("range", "vertex", "normal"))
        self.range[1].copy_(m["range"][0])
        self.vertex[1].copy_(m["vertex"][0])
        self.normal[1].copy_(m["normal"][0])

    def _deskewed(self, pts, times, t_from: np.ndarray, t_to: np.ndarray):
        """The raw scan `pts` (a device tensor) under the twist of the step t_from -> t_to, as a new device tensor."""
        import torch
        from .deskew import deskew_scans, se3_log, source_of
        xi = se3_log(np.linalg.inv(t_from) @ t_to)
        self._offs[1] = int(pts.shape[0])
        return deskew_scans(self.engine, pts, self._offs, torch.from_numpy(xi[None]).to(self.engine.device),
                            t_ref=self.deskew["t_ref"], **source_of(self.deskew, times, "track"))

    def _rebuild_seed(self) -> None:
        """Before scan 2 is tracked: the model, which so far holds scans 0 and 1 as they came, is rebuilt from them deskewed by the
        first step Log(T_0^-1 T_1), the motion estimate that now exists for both.  Left as they came they would bend the model every
        deskewed scan is registered onto.  Slot 2 ends up holding scan 1 as it was fused."""
        import torch
        seed, self._seed = self._seed, []
        fused = [r.source != SOURCE_PREDICTION for r in self.results[:2]]
        self.volume.reset()
        for (raw, times), pose, was_fused in zip(seed, self.poses[:2], fused):
            if raw is None or not was_fused:
                continue
            self._project(self._deskewed(raw, times, self.poses[0], self.poses[1]))
            self._fuse(torch.from_numpy(np.ascontiguousarray(pose[None])).to(self.engine.device))
        if seed[1][0] is not None and fused[1]:
            for t in (self.range, self.vertex, self.normal):
                t[2].copy_(t[1])

    def _fuse(self, pose_dev) -> None:
        up, down, rmax = self.sensor
        v = self.volume
        self.engine.tsdf_integrate(v.tsdf, v.weight, v.origin, v.voxel, v.trunc, v.max_weight, self.range[1:2], pose_dev, up, down, rmax,
                                   **v._window())
        v.n_scans += 1

    def track(self, points, first_pose=None, times=None) -> TrackResult:
        """One scan, (N,4) float32 sensor-frame points (host array or device tensor).  first_pose: the pose of the FIRST scan (the
        identity by default); refused on a later one.  times: with `deskew`, the (N,) float32 time fraction of every point within
        the sweep (host array or device tensor); without them the deskew dict's azimuth parameters give the times."""
        import torch
        shape = tuple(points.shape)
        if len(shape) != 2 or shape[1] != 4:
            raise ValueError("points must be (N,4), got %s" % (shape,))
        if self.poses and first_pose is not None:
            raise ValueError("first_pose belongs to the first scan; %d are tracked" % len(self.poses))
        dev = self.engine.device
        raw = None                                   # with deskew: the raw scan on the device, for scans that have a motion estimate
        if self.deskew is None:
            if times is not None:
                raise ValueError("times belong to a tracker built with deskew=")
        else:
            from .deskew import source_of, times_tensor
            source_of(self.deskew, times, "track")                                       # refuses a scan without a time source
            if times is not None:
                times = times_tensor(self.engine, times, shape[0], "track")
            if shape[0] > 0:
                raw = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, np.float32))
                raw = raw.to(dev, torch.float32).contiguous()
            if len(self.poses) < 2:
                self._seed.append((raw, times))                                          # scans 0 and 1, kept until scan 2 arrives
            elif len(self.poses) == 2:
                self._rebuild_seed()
        up, down, rmax = self.sensor
        if not self.poses:
            pose = np.eye(4) if first_pose is None else np.array(first_pose, np.float64).reshape(4, 4)
            if not np.isfinite(pose).all():
                raise ValueError("first_pose is not finite")
            self._project(points)
            self._before_view(pose)
            self._fuse(torch.from_numpy(pose[None]).to(dev))
            res = TrackResult(pose, SOURCE_FIRST, 0, 0.0, 0.0, 0)
        else:
            t_last = self.poses[-1]
            t_pred = predict(self.poses[-2], t_last) if len(self.poses) > 1 else t_last.copy()
            if raw is not None:
                points = self._deskewed(raw, times, self.poses[-2], t_last) if len(self.poses) > 1 else raw
            self._project(points)
            both = torch.from_numpy(np.stack([t_pred, t_last])).to(dev)                      # what each registration's result multiplies
            self._before_view(t_pred)
            v = self.volume
            mask = self.engine.tsdf_bricks(v.weight, self.min_weight) if self.use_bricks else None
            self.engine.tsdf_raycast(v.tsdf, v.weight, v.origin, v.voxel, both[0:1], self.h, self.w, up, down, self.min_range, rmax,
                                     v.voxel, self.min_weight, mask, want=(),
                                     out=dict(range=self.range[0:1], vertex=self.vertex[0:1], normal=self.normal[0:1]), **v._window())
            icp, stats = self.engine.icp_register(self.vertex, self.normal, self.range, self._src, self._tgt, self._init, fov_up=up,
                                                  fov_down=down, max_range=rmax, **self.icp_params)
            # pose candidates: prediction . model registration, last pose . frame registration, the prediction itself
            world = (both[:, :, :, None] * icp[:, None, :, :]).sum(dim=2)
            ok = stats[:, 0] == 0
            if self.min_fitness is not None:
                ok = ok & (stats[:, 2] >= self.min_fitness * stats[:, 3]) & (stats[:, 3] > 0)
            pick = torch.where(ok[0], 0, torch.where(ok[1], 1, 2))
            cand = torch.cat([world, both[0:1]], dim=0)
            chosen = cand[pick]
            row = torch.cat([chosen.reshape(16), stats[torch.clamp(pick, max=1)], pick.to(torch.float64).reshape(1)])
            back = row.cpu().numpy()                                                         # the frame's one read-back
            pose, st, which = back[:16].reshape(4, 4).copy(), back[16:24], int(back[24])
            valid = int(st[3])
            res = TrackResult(pose, _SOURCES[which], int(st[0]), (st[2] / valid) if valid > 0 else 0.0, float(st[4]), int(st[2]))
            if which != 2:
                if raw is not None and self.deskew_passes == 2:
                    self._project(self._deskewed(raw, times, t_last, pose))               # the images that are fused and kept in slot 2
                self._fuse(chosen.reshape(1, 4, 4).contiguous())
        for t in (self.range, self.vertex, self.normal):
            t[2].copy_(t[1])
        self.poses.append(res.pose)
        self.results.append(res)
        return res


class RollingTsdfOdometry(TsdfOdometry):
    """`TsdfOdometry` against a volume that follows the sensor (`tsdf.RollingTsdfVolume`): online, with memory
    and a frame's cost that do not depend on the length of the drive.

    extent: the window's size in metres, 3 numbers or one for all axes; anchor: the lattice's fixed point; shift: the voxels the window
    moves at a time, a multiple of 8.  Before a scan's view is cast -- before the first scan is fused -- the window follows the
    predicted position; the cells that leave are meshed and go to on_leave(piece (T,3,3) float32), or into `volume.pieces` without one,
    so that `volume.mesh()` is the whole drive's.  Refused: a window whose half extent in x or y is below max_range + trunc + voxel +
    shift * voxel, what a scan can reach from a sensor that may stand `shift` voxels off the centre.  The z extent is the caller's to
    choose, as `below` and `above` are for the fixed box: a sensor that looks along the ground does not reach max_range upwards.
    store: the volume's (`RollingTsdfVolume(store=)`) -- True or a `tsdf_store.TsdfBrickStore` keeps what leaves
    the window and brings it back when the drive returns; nothing is meshed on the way, so on_leave is refused with it."""

    def __init__(self, engine, extent, voxel: float, trunc: Optional[float] = None, anchor=(0.0, 0.0, 0.0), shift: int = 8,
                 on_leave=None, store=None, **tracker):
        if store is not None and store is not False and on_leave is not None:
            raise ValueError("on_leave and store= exclude each other: with a store nothing is meshed when it leaves")
        self._rolling = dict(extent=extent, anchor=anchor, shift=shift, store=store)
        self.on_leave = on_leave
        super().__init__(engine, None, None, voxel, trunc=trunc, **tracker)

    def _make_volume(self, engine, lo, hi, voxel, trunc, max_weight, max_range):
        from .tsdf import DEFAULT_TRUNC_VOXELS, RollingTsdfVolume, window_shape
        shape = window_shape(self._rolling["extent"], voxel)
        shift = self._rolling["shift"]
        tr = DEFAULT_TRUNC_VOXELS * float(voxel) if trunc is None else float(trunc)
        need = max_range + tr + float(voxel) + float(shift) * float(voxel)
        half = min(shape[0], shape[1]) // 2 * float(voxel)
        if not half >= need:
            raise ValueError("a window of %d x %d samples at voxel %g m reaches %g m from its centre in x or y, below max_range + trunc + "
                             "voxel + shift * voxel = %g m" % (shape[0], shape[1], voxel, half, need))
        return RollingTsdfVolume(engine, self._rolling["extent"], voxel, trunc=trunc, max_weight=max_weight,
                                 anchor=self._rolling["anchor"], shift=shift, store=self._rolling["store"])

    def _before_view(self, pose: np.ndarray) -> None:
        self.volume.follow(np.asarray(pose, np.float64)[:3, 3], self.on_leave, self.min_weight)


def estimate_poses(engine, points, offsets, voxel: float = 0.2, trunc: Optional[float] = None, proj_h: int = 64, proj_w: int = 900,
                   fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0, min_range: float = 0.5, below: float = 5.0,
                   above: float = 15.0, chunk: int = 64, min_fitness: Optional[float] = None, window=None, shift: int = 8,
                   deskew: Optional[dict] = None, times=None, deskew_passes: int = 1, keep: bool = False, **icp_params):
    """The poses of a drive from its scans: `frame_to_frame` gives a first trajectory, its `bounds_from_poses` the volume's box, and
    `TsdfOdometry` tracks the drive against the volume it builds.  A box over 2^31 - 1 samples is refused with `volume_shape`'s message,
    which names the voxel that fits (the volume does not follow the sensor).  -> (poses (n,4,4), [TrackResult] * n, the TsdfVolume).
    window: metres, 3 numbers or one for x and y with below + above for z -- `RollingTsdfOdometry` tracks the drive in a window of
    that size that follows the sensor, `shift` voxels at a time: no `frame_to_frame` pass, no limit on the drive's extent, and the
    volume returned is the RollingTsdfVolume, whose `mesh()` is the whole drive's.  keep=True (with window) gives that volume a brick
    store: what leaves the window is kept and comes back when the drive revisits it.
    deskew, deskew_passes: the trackers' (DESIGN.md section 37), with times (total,) float32, one fraction per row of `points`, where
    the deskew dict names no azimuth parameters.  `frame_to_frame` does not deskew: its trajectory only sizes the box."""
    from .tsdf import volume_shape
    offs = _check_scans(points, offsets)
    n = offs.shape[0] - 1
    if n < 1:
        raise ValueError("estimate_poses needs at least one scan")
    if keep and window is None:
        raise ValueError("keep=True belongs to window=: the fixed box forgets nothing")
    if times is not None:
        if deskew is None:
            raise ValueError("times belong to deskew=")
        if tuple(times.shape) != (int(points.shape[0]),):
            raise ValueError("times must hold one fraction per point, (%d,), got %s" % (int(points.shape[0]), tuple(times.shape)))
    scan_times = lambda s: {} if times is None else dict(times=times[int(offs[s]):int(offs[s + 1])])
    motion = dict(deskew=deskew, deskew_passes=deskew_passes)
    sensor = dict(proj_h=proj_h, proj_w=proj_w, fov_up=fov_up, fov_down=fov_down, max_range=max_range)
    if window is not None:
        ext = np.asarray(window, np.float64).reshape(-1)
        if ext.shape[0] == 1:
            ext = np.array([ext[0], ext[0], float(below) + float(above)])
        odo = RollingTsdfOdometry(engine, ext, voxel, trunc=trunc, shift=shift, min_range=min_range, min_fitness=min_fitness,
                                  store=True if keep else None, **sensor, **motion, **icp_params)
        for s in range(n):
            odo.track(points[int(offs[s]):int(offs[s + 1])], **scan_times(s))
        return np.stack(odo.poses), odo.results, odo.volume
    first, _ = frame_to_frame(engine, points, offsets, chunk=chunk, **sensor, **icp_params)
    lo, hi = bounds_from_poses(first, max_range, below, above)
    volume_shape(lo, hi, voxel)
    odo = TsdfOdometry(engine, lo, hi, voxel, trunc=trunc, min_range=min_range, min_fitness=min_fitness, **sensor, **motion,
                       **icp_params)
    for s in range(n):
        odo.track(points[int(offs[s]):int(offs[s + 1])], **scan_times(s))
    return np.stack(odo.poses), odo.results, odo.volume
