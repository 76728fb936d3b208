"""Motion compensation of raw LiDAR sweeps (ovn_deskew, include/ovn_hip_deskew.h, csrc/deskew.hip).

    xi = twists_from_poses(poses)                                     # (n,6) body-frame twists (v, omega), one per sweep
    pts = deskew_scans(engine, points, offsets, xi, times=fractions)  # or start_azimuth=..., clockwise=... without per-point times

A spinning sensor measures the points of a sweep one after the other while it moves.  With the motion over a sweep given as a constant
twist and each point's time as a fraction of the sweep, `deskew_scans` expresses every point in the frame the sensor had at fraction
`t_ref`.  The SE(3) helpers are NumPy float64 and run on the host; the points are moved by one HIP kernel.  Nothing here is on by
default anywhere: `odometry`, `tsdf` and the tools take a `deskew` configuration (`check_config`) and leave every call as it was
without one.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np

SERIES_BELOW = 0.1           # |omega| under which the fp64 coefficients of se3_exp / se3_log are their series
CONFIG_KEYS = ("t_ref", "start_azimuth", "clockwise")


def _finite_f32(x) -> bool:
    with np.errstate(over="ignore"):
        return bool(np.isfinite(np.float32(float(x))))


def _hat(w: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _exp_coefficients(th: float):
    """(A, B, C) = (sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3), by their series below SERIES_BELOW."""
    t2 = th * th
    if th < SERIES_BELOW:
        a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0 * (1.0 - t2 / 110.0))))
        b = 0.5 * (1.0 - t2 / 12.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0 * (1.0 - t2 / 90.0 * (1.0 - t2 / 132.0)))))
        c = 1.0 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0 * (1.0 - t2 / 110.0 * (1.0 - t2 / 156.0)))))
        return a, b, c
    sh = np.sin(0.5 * th)
    return np.sin(th) / th, 2.0 * sh * sh / t2, (th - np.sin(th)) / (t2 * th)


def se3_exp(xi) -> np.ndarray:
    """The 4 x 4 transform Exp(xi) of a twist xi = (v, omega): R = I + A K + B K^2, t = (I + B K + C K^2) v with K = [omega]x."""
    xi = np.asarray(xi, np.float64).reshape(6)
    v, w = xi[:3], xi[3:]
    a, b, c = _exp_coefficients(float(np.sqrt(w @ w)))
    k = _hat(w)
    kk = k @ k
    t = np.eye(4)
    t[:3, :3] = np.eye(3) + a * k + b * kk
    t[:3, 3] = v + b * (k @ v) + c * (kk @ v)
    return t


def se3_log(t) -> np.ndarray:
    """The twist (v, omega) with Exp(twist) = t, for a rotation angle below pi."""
    t = np.asarray(t, np.float64).reshape(4, 4)
    r = t[:3, :3]
    s = 0.5 * np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])        # sin th * axis
    sn = float(np.sqrt(s @ s))
    th = float(np.arctan2(sn, 0.5 * (np.trace(r) - 1.0)))
    w = s * (th / sn) if sn > 1e-8 else s.copy()           # th / sin th = 1 + th^2 / 6 + ..: 1 to 1e-17 below
    t2 = th * th
    if th < SERIES_BELOW:                                  # D = (1 - (th / 2) cot(th / 2)) / th^2
        d = 1.0 / 12.0 * (1.0 + t2 / 60.0 * (1.0 + t2 / 42.0 * (1.0 + t2 / 40.0 * (1.0 + t2 * 10.0 / 396.0))))
    else:
        d = (1.0 - 0.5 * th / np.tan(0.5 * th)) / t2
    k = _hat(w)
    p = t[:3, 3]
    return np.concatenate([p - 0.5 * (k @ p) + d * (k @ (k @ p)), w])


def twists_from_poses(poses) -> np.ndarray:
    """(n,6): xi_k = Log(T_{k-1}^-1 T_k) for k >= 1 -- the step that brought the sensor to pose k, taken as its motion over sweep k --
    and xi_0 = xi_1.  A single pose gives zeros."""
    p = np.asarray(poses, np.float64)
    if p.ndim != 3 or p.shape[1:] != (4, 4):
        raise ValueError("poses must be (n,4,4), got %s" % (p.shape,))
    out = np.zeros((p.shape[0], 6))
    for k in range(1, p.shape[0]):
        out[k] = se3_log(np.linalg.inv(p[k - 1]) @ p[k])
    if p.shape[0] > 1:
        out[0] = out[1]
    return out


def check_config(deskew) -> Optional[dict]:
    """The `deskew=` argument of `odometry` and `tsdf` as a dict with every key of CONFIG_KEYS, or None for None.  t_ref defaults to
    0.5: under a mis-estimated twist a point's error grows with |s - t_ref|, and the middle of the sweep minimises its maximum.
    start_azimuth (degrees) and clockwise have no defaults -- where a sweep starts and which way it turns is a property of the sensor
    -- and come together or not at all; without them every scan needs its per-point times."""
    if deskew is None:
        return None
    if not isinstance(deskew, dict):
        raise ValueError("deskew must be None or a dict with keys among %s, got %r" % (CONFIG_KEYS, deskew))
    bad = [k for k in deskew if k not in CONFIG_KEYS]
    if bad:
        raise ValueError("unknown deskew keys %s (known: %s)" % (bad, list(CONFIG_KEYS)))
    t_ref = float(deskew.get("t_ref", 0.5))
    if not _finite_f32(t_ref):
        raise ValueError("deskew t_ref must be a finite number, got %r" % (deskew.get("t_ref"),))
    az, cw = deskew.get("start_azimuth"), deskew.get("clockwise")
    if (az is None) != (cw is None):
        raise ValueError("deskew start_azimuth and clockwise come together: got start_azimuth=%r, clockwise=%r" % (az, cw))
    if az is not None:
        _check_azimuth(az, cw)
        az, cw = float(az), bool(cw)
    return dict(t_ref=t_ref, start_azimuth=az, clockwise=cw)


def _check_azimuth(start_azimuth, clockwise) -> None:
    if not np.isfinite(float(start_azimuth)):
        raise ValueError("start_azimuth must be a finite number of degrees, got %r" % (start_azimuth,))
    if clockwise not in (0, 1, False, True):
        raise ValueError("clockwise must be True or False, got %r" % (clockwise,))


def source_of(cfg: dict, times, what: str) -> dict:
    """The time-source arguments of `deskew_scans` for one call under the configuration `cfg`: the given times, else the configured
    azimuth parameters; ValueError when there is neither."""
    if times is not None:
        return dict(times=times)
    if cfg["start_azimuth"] is None:
        raise ValueError("%s: deskew needs a time source: per-point times, or start_azimuth and clockwise in the deskew dict" % what)
    return dict(start_azimuth=cfg["start_azimuth"], clockwise=cfg["clockwise"])


def times_tensor(engine, times, n_points: int, what: str):
    """Per-point time fractions (host array or tensor) as a contiguous float32 tensor of n_points elements on the engine's device."""
    import torch
    shape = tuple(times.shape) if hasattr(times, "shape") else tuple(np.shape(times))
    if len(shape) != 1 or shape[0] != int(n_points):
        raise ValueError("%s: times must hold one fraction per point, (%d,), got %s" % (what, int(n_points), shape))
    t = times if isinstance(times, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(times, np.float32))
    return t.to(engine.device, torch.float32).contiguous()


def deskew_scans(engine, points, offsets, twists, times=None, start_azimuth=None, clockwise=None, t_ref: float = 0.5, out=None):
    """Every point of raw sweeps in the sensor frame of fraction `t_ref` of its sweep (ovn_deskew) -> a (total,4) float32 device tensor.

    points (total,4) float32 and offsets (n+1) int64 device tensors as for `engine.project` (absolute rows; rows outside
    offsets[0] .. offsets[n] are not touched: in a fresh result they are uninitialised).  twists (n,6) float64, a device tensor or a host
    array: the sensor's body-frame twist (v, omega) over each whole sweep.  times (total,) float32 device tensor of each point's
    fraction of its sweep, 0 its first point and 1 its last; without it the time comes from the azimuth, and start_azimuth (degrees,
    the projection's yaw -atan2(y, x) at which a sweep starts) and clockwise (whether that yaw grows with time) are both required:
    they have no defaults, because nobody here has measured a sensor.  out: the result's tensor; `points` itself deskews in place,
    a tensor that shares only part of its memory with `points` is refused."""
    import torch
    from . import _lib
    from .engine import _ptr
    engine._check(points, "deskew_scans: points", ndim=2)
    if points.shape[1] != 4:
        raise _lib.OvnError("deskew_scans: points must be (total,4), got %s" % (tuple(points.shape),))
    engine._check(offsets, "deskew_scans: offsets", torch.int64, ndim=1)
    n = offsets.numel() - 1
    if n < 0:
        raise _lib.OvnError("deskew_scans: offsets must hold n + 1 >= 1 entries")
    if not isinstance(twists, torch.Tensor):
        twists = torch.from_numpy(np.ascontiguousarray(np.asarray(twists, np.float64).reshape(-1, 6))).to(engine.device)
    engine._check(twists, "deskew_scans: twists", torch.float64, (n, 6))
    total = int(points.shape[0])
    engine._check(times, "deskew_scans: times", shape=(total,), optional=True)
    if times is None:
        if start_azimuth is None or clockwise is None:
            raise ValueError("deskew_scans: without times, start_azimuth and clockwise are both required (they have no defaults)")
        _check_azimuth(start_azimuth, clockwise)
    elif start_azimuth is not None or clockwise is not None:
        raise ValueError("deskew_scans: times and the azimuth parameters are two time sources: give one")
    if not _finite_f32(t_ref):
        raise ValueError("deskew_scans: t_ref must be a finite number, got %r" % (t_ref,))
    if out is None:
        out = torch.empty_like(points)
    else:
        engine._check(out, "deskew_scans: out", shape=(total, 4))
        gap = abs(out.data_ptr() - points.data_ptr())
        if 0 < gap < 16 * total:
            raise _lib.OvnError("deskew_scans: out overlaps points without being points (in place)")
    engine._call("ovn_deskew", engine._stream(), _ptr(points), _ptr(offsets), n, _ptr(times),
                 0.0 if start_azimuth is None else float(start_azimuth), int(bool(clockwise)), _ptr(twists), float(t_ref), _ptr(out))
    return out


# ---- what the three tools share ----------------------------------------------------------------------------------------------------
def add_arguments(ap) -> None:
    """--deskew and its time source on an argparse parser (tools/odometry.py, tools/build_mesh.py, tools/slam.py)."""
    ap.add_argument("--deskew", action="store_true", help="the scans are raw sweeps: undo the sensor's motion within each (needs "
                    "--times, or --start-azimuth with --clockwise or --counter-clockwise)")
    ap.add_argument("--times", default=None, metavar="DIR", help="folder with one NNNNNN.npy or float32 NNNNNN.bin per scan: each "
                    "point's time as a fraction of its sweep")
    ap.add_argument("--start-azimuth", type=float, default=None, metavar="DEG", help="the yaw -atan2(y, x) at which a sweep starts")
    turn = ap.add_mutually_exclusive_group()
    turn.add_argument("--clockwise", dest="clockwise", action="store_const", const=True, default=None,
                      help="that yaw grows with time (the sensor turns clockwise seen from above)")
    turn.add_argument("--counter-clockwise", dest="clockwise", action="store_const", const=False)
    ap.add_argument("--t-ref", type=float, default=0.5, help="the fraction of a sweep whose sensor frame a deskewed scan is in")


def config_from_args(ap, a) -> Optional[dict]:
    """The `deskew=` dict of the parsed arguments, None without --deskew; a missing or doubled time source is an argparse error."""
    azimuth = a.start_azimuth is not None or a.clockwise is not None
    if not a.deskew:
        if a.times is not None or azimuth:
            ap.error("--times, --start-azimuth, --clockwise and --counter-clockwise belong to --deskew")
        return None
    if a.times is None and not azimuth:
        ap.error("--deskew needs a time source: --times DIR, or --start-azimuth DEG with --clockwise or --counter-clockwise")
    if a.times is not None and azimuth:
        ap.error("--times and --start-azimuth are two time sources: give one")
    if a.times is None and (a.start_azimuth is None or a.clockwise is None):
        ap.error("--start-azimuth DEG and one of --clockwise, --counter-clockwise come together")
    try:
        return check_config(dict(t_ref=a.t_ref, start_azimuth=a.start_azimuth, clockwise=a.clockwise))
    except ValueError as e:
        ap.error(str(e))


def read_times(folder: str, scan_paths, counts) -> np.ndarray:
    """The concatenated float32 time fractions of the scans at `scan_paths`: <folder>/<scan name>.npy, else .bin (raw float32), each
    checked against its scan's number of points (`counts`)."""
    parts = []
    for path, n in zip(scan_paths, counts):
        stem = os.path.splitext(os.path.basename(path))[0]
        npy, raw = os.path.join(folder, stem + ".npy"), os.path.join(folder, stem + ".bin")
        if os.path.isfile(npy):
            t = np.load(npy)
        elif os.path.isfile(raw):
            t = np.fromfile(raw, dtype=np.float32)
        else:
            raise ValueError("no times for scan %s: neither %s nor %s exists" % (stem, npy, raw))
        if t.ndim != 1 or t.shape[0] != int(n):
            raise ValueError("%s holds times of shape %s for a scan of %d points" % (npy if os.path.isfile(npy) else raw, t.shape, int(n)))
        parts.append(np.asarray(t, np.float32))
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)
