"""Geometric verification of loop-closure candidates: the yaw head's angle seeds a frame-to-frame ICP on the range images, and the
registration's fitness and residual say whether the loop holds up (the step the OverlapNet paper takes after the network).  The ICP
is one HIP kernel for all pairs of a call (`ovn_icp_register`, csrc/icp_register.hip); this module is the plumbing around it."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import OvnEngine

STATUS_OK, STATUS_STOPPED, STATUS_BAD_INDEX = 0, 1, 2


class Registration(NamedTuple):
    pose: np.ndarray                   # (4,4) f64: source-frame points into the target frame
    fitness: float                     # inliers / valid source pixels
    rms: float                         # sqrt(sum w r^2 / inliers) of the point-to-plane residuals at `pose` [m]
    status: int                        # 0 ok; 1 stopped early (too few inliers / singular system); 2 index out of range
    last_step: Tuple[float, float]     # |v| [m] and |omega| [rad] of the last update: small when the iteration has settled
    inliers: int
    valid: int


def pose_from_yaw_bin(bin, width: int = 360) -> np.ndarray:
    """Rz(phi), phi = (width / 2 - bin) * 360 / width degrees, as a 4x4 pose, for a GROUND-TRUTH yaw bin: the value
    com_overlap_yaw.py:48-55 writes into a row [current, reference, overlap, bin].  It is the rotation that takes REFERENCE-scan
    points into the CURRENT scan's frame -- the initial pose of an ICP whose source is the reference scan and whose target is the
    current scan.  This is NOT the yaw `Infer` returns: that is 180 - argmax, with the legs the other way round; use
    `pose_from_network_yaw` for it."""
    phi = np.radians((width / 2.0 - float(bin)) * 360.0 / width)
    c, s = np.cos(phi), np.sin(phi)
    T = np.eye(4)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    return T


def pose_from_network_yaw(yaw, width: int = 360) -> np.ndarray:
    """The initial pose (reference scan = source into current scan = target) from the yaw `Infer.infer_multiple`, `infer_top_k`
    and `infer_best_match` return for a (reference, current) pair.  That yaw is 180 - argmax of the correlation (infer.py:158), and
    `Infer` puts the REFERENCE on the first leg and the current frame on the second (infer.py:188-190), the other way round than
    the training pairs [current, reference] whose label is the ground-truth bin.  So argmax is the ground-truth bin of the swapped
    pair, the rotation taking CURRENT-scan points into the REFERENCE frame, and the pose wanted here is its inverse:
    pose_from_yaw_bin(180 - yaw, width) transposed -- Rz(-yaw degrees) at the shipped width of 360."""
    return np.ascontiguousarray(pose_from_yaw_bin(180 - float(yaw), width).T)


def decode_registrations(pose: torch.Tensor, stats: torch.Tensor) -> List[Registration]:
    P, S = pose.cpu().numpy(), stats.cpu().numpy()
    out = []
    for p, s in zip(P, S):
        inl, valid = int(s[2]), int(s[3])
        out.append(Registration(p, inl / valid if valid > 0 else 0.0, float(s[4]), int(s[0]), (float(s[5]), float(s[6])), inl, valid))
    return out


def register_scans(engine: OvnEngine, points: Sequence[np.ndarray], pairs, init_poses, proj_H: int = 64, proj_W: int = 900,
                   fov_up: float = 3.0, fov_down: float = -25.0, max_range: float = 50.0, **params) -> List[Registration]:
    """Project the raw (N_i,4) clouds once and register every (source, target) index pair of `pairs` from its initial pose
    (`init_poses`: (P,4,4), source into target) in one launch.  **params: iterations, max_dist, cos_min, huber, min_inliers."""
    from .preprocess import project_scans
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    init = np.ascontiguousarray(np.asarray(init_poses, dtype=np.float64).reshape(-1, 4, 4))
    if init.shape[0] != pairs.shape[0]:
        raise ValueError("register_scans: %d pairs but %d initial poses" % (pairs.shape[0], init.shape[0]))
    if pairs.shape[0] == 0:
        return []
    r = project_scans(points, engine=engine, proj_H=proj_H, proj_W=proj_W, fov_up=fov_up, fov_down=fov_down, max_range=max_range,
                      want=("range", "vertex", "normal"))
    dev = engine.device
    src = torch.from_numpy(pairs[:, 0].astype(np.int32)).to(dev)
    tgt = torch.from_numpy(pairs[:, 1].astype(np.int32)).to(dev)
    pose, stats = engine.icp_register(r["vertex"], r["normal"], r["range"], src, tgt, torch.from_numpy(init).to(dev),
                                      fov_up=fov_up, fov_down=fov_down, max_range=max_range, **params)
    return decode_registrations(pose, stats)


def accept(reg: Registration, min_fitness: Optional[float] = None, max_rms: Optional[float] = None) -> Optional[bool]:
    """None when no threshold is given (no default is chosen here: none has been measured on real loop closures); else whether
    the registration finished (status 0) and meets every threshold given."""
    if min_fitness is None and max_rms is None:
        return None
    ok = reg.status == STATUS_OK
    if min_fitness is not None:
        ok = ok and reg.fitness >= min_fitness
    if max_rms is not None:
        ok = ok and reg.rms <= max_rms
    return bool(ok)
