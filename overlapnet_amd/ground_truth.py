"""Ground-truth overlap / yaw labels on the GPU -- drop-in for the reference's `src/utils/com_overlap_yaw.py`.

`com_overlap_yaw(scan_paths, poses, frame_idx, leg_output_width=360)` has the reference's signature and return value
(rows `[current_frame_idx, reference_frame_idx, overlap, yaw_bin]`, com_overlap_yaw.py:10-68); the N float64 range
projections of the transformed reference clouds (the O(N x 125k points) part) run in `csrc/overlap_gt.hip`, the yaw bin
is scalar host arithmetic restated operator for operator (Python precedence included).  `OverlapGroundTruth` keeps the
scans resident in HBM so that labelling every frame of a sequence (demo4 labels one, training wants all) costs one
upload: 1101 KITTI scans = 2.2 GB.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .engine import OvnEngine


def load_vertex(scan_path: str) -> np.ndarray:
    """(n,4) float64 homogeneous points (x, y, z, 1) of a KITTI .bin scan (utils.py:217-230)."""
    cur = np.fromfile(scan_path, dtype=np.float32).reshape((-1, 4))
    out = np.ones((cur.shape[0], 4))
    out[:, :3] = cur[:, :3]
    return out


def euler_angles_from_rotation_matrix(R):
    """(roll, pitch, yaw) after Slabaugh, utils.py:186-214."""
    def isclose(x, y, rtol=1.e-5, atol=1.e-8):
        return abs(x - y) <= atol + rtol * abs(y)

    phi = 0.0
    if isclose(R[2, 0], -1.0):
        theta = math.pi / 2.0
        psi = math.atan2(R[0, 1], R[0, 2])
    elif isclose(R[2, 0], 1.0):
        theta = -math.pi / 2.0
        psi = math.atan2(-R[0, 1], -R[0, 2])
    else:
        theta = -math.asin(R[2, 0])
        cos_theta = math.cos(theta)
        psi = math.atan2(R[2, 1] / cos_theta, R[2, 2] / cos_theta)
        phi = math.atan2(R[1, 0] / cos_theta, R[0, 0] / cos_theta)
    return psi, theta, phi


def yaw_bin(current_pose: np.ndarray, reference_pose: np.ndarray, yaw_resolution: int = 360) -> int:
    """com_overlap_yaw.py:49-55.  Note `-(yaw / pi) * W // 2 + W // 2`: the floor division applies to the product."""
    relative_transform = np.linalg.inv(current_pose).dot(reference_pose)
    _, _, yaw = euler_angles_from_rotation_matrix(relative_transform[:3, :3])
    return int(-(yaw / np.pi) * yaw_resolution // 2 + yaw_resolution // 2)


def _yaw_bin_of(relative_transform: np.ndarray, yaw_resolution: int) -> int:
    _, _, yaw = euler_angles_from_rotation_matrix(relative_transform[:3, :3])
    return int(-(yaw / np.pi) * yaw_resolution // 2 + yaw_resolution // 2)


def yaw_bins_all(poses: np.ndarray, frames: Optional[Sequence[int]] = None, refs: Optional[Sequence[int]] = None,
                 yaw_resolution: int = 360) -> np.ndarray:
    """(F, R) int64: `yaw_bin(poses[frames[f]], poses[refs[r]], yaw_resolution)` for every pair, element for element.

    One host inversion per frame.  The relative rotation's three entries the yaw needs are formed for all references at once and
    binned in NumPy; that arithmetic is not the scalar function's bit for bit (another summation order in the product, libm
    against NumPy's loops), and the bin is a floor, so every pair the difference could move is recomputed with the scalar
    arithmetic: `-(yaw / pi) * W / 2` within 1e-6 of an integer (two poses with the same rotation put it at +-1e-16: straight
    driving lands here), R[2,0] within 1e-4 of +-1 (gimbal lock, where the scalar function leaves the yaw at 0; its own
    tolerance is 1e-5) and anything not finite.  The two evaluations differ by a few ulp of values below 4, far inside 1e-6."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    frames = np.arange(len(poses)) if frames is None else np.asarray(frames, np.int64).reshape(-1)
    refs = np.arange(len(poses)) if refs is None else np.asarray(refs, np.int64).reshape(-1)
    out = np.zeros((len(frames), len(refs)), np.int64)
    if out.size == 0:
        return out
    ref_poses = poses[refs]
    col0 = ref_poses[:, :, 0]                                   # (R, 4): first column of every reference pose
    half = yaw_resolution // 2
    for i, f in enumerate(frames):
        inv = np.linalg.inv(poses[f])
        r00, r10, r20 = col0 @ inv[0], col0 @ inv[1], col0 @ inv[2]
        with np.errstate(all="ignore"):
            cos_theta = np.cos(-np.arcsin(r20))
            yaw = np.arctan2(r10 / cos_theta, r00 / cos_theta)
            v = -(yaw / np.pi) * yaw_resolution
            t = v / 2.0
            redo = ~np.isfinite(t) | (np.abs(t - np.rint(t)) < 1e-6) | (np.abs(np.abs(r20) - 1.0) < 1e-4)
            bins = np.floor(np.where(redo, 0.0, t)).astype(np.int64) + half
        for r in np.nonzero(redo)[0]:
            bins[r] = _yaw_bin_of(inv.dot(ref_poses[r]), yaw_resolution)
        out[i] = bins
    return out


class OverlapGroundTruth:
    """Scans resident on the device; `mapping(frame_idx)` = the reference's ground_truth_mapping for that frame."""

    def __init__(self, scans: Sequence[np.ndarray], poses: np.ndarray, engine: Optional[OvnEngine] = None,
                 leg_output_width: int = 360, proj_H: int = 64, proj_W: int = 900, fov_up: float = 3.0,
                 fov_down: float = -25.0, max_range: float = 50.0):
        if len(scans) != len(poses):
            raise Exception("need one pose per scan (%d scans, %d poses)" % (len(scans), len(poses)))
        self.engine = engine or OvnEngine(proj_H, proj_W, 1)
        self.poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
        self.n = len(scans)
        self.leg_output_width = leg_output_width
        self.proj = dict(proj_h=proj_H, proj_w=proj_W, fov_up=fov_up, fov_down=fov_down, max_range=max_range)
        sizes = [int(np.asarray(s).shape[0]) for s in scans]
        self.max_points = max(sizes) if sizes else 0
        off = np.zeros(self.n + 1, np.int64)
        off[1:] = np.cumsum(sizes)
        pts = np.zeros((int(off[-1]), 4), np.float32)
        for i, s in enumerate(scans):
            pts[off[i]:off[i + 1], :3] = np.asarray(s)[:, :3]      # load_vertex keeps x, y, z only (utils.py:226-229)
        dev = self.engine.device
        self._points = torch.from_numpy(pts).to(dev)
        self._offsets = torch.from_numpy(off).to(dev)
        self._ref_poses = torch.from_numpy(np.ascontiguousarray(self.poses)).to(dev)
        self._host_offsets = off
        self._cur = None                                        # own range images and inverse poses: all_pairs fills them
        self._valid = None
        self._inv_poses = None

    def overlaps(self, frame_idx: int) -> np.ndarray:
        """(n,) float64 overlap of every scan with frame `frame_idx` (com_overlap_yaw.py:28-46)."""
        e = self.engine
        lo, hi = int(self._offsets[frame_idx]), int(self._offsets[frame_idx + 1])
        one = torch.tensor([0, hi - lo], dtype=torch.int64, device=e.device)
        cur = e.gt_range_images(self._points[lo:hi], one, hi - lo, **self.proj)
        inv_cur = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(self.poses[frame_idx]))).to(e.device)
        counts = None
        chunk = 512                                            # 512 range images = 118 MB of scratch per pass
        out = np.zeros(self.n)
        valid = 0
        for s0 in range(0, self.n, chunk):
            s1 = min(self.n, s0 + chunk)
            off = (self._offsets[s0:s1 + 1] - self._offsets[s0]).contiguous()
            p0, p1 = int(self._offsets[s0]), int(self._offsets[s1])
            imgs = e.gt_range_images(self._points[p0:p1], off, self.max_points, self._ref_poses[s0:s1].contiguous(), inv_cur,
                                     **self.proj)
            counts = e.gt_overlap_counts(imgs, cur).cpu().numpy()
            out[s0:s1] = counts[:-1]
            valid = int(counts[-1])
        if self.n and valid == 0:
            raise ZeroDivisionError("frame %d has no point inside the field of view" % frame_idx)
        return out / valid if self.n else out

    def _own_ranges(self, scans: np.ndarray):
        """Own range images (n, H, W) f32 on the device and their `valid_num` (n,) int64 on the host, filled for `scans` and
        kept: a scan's image is computed once per object."""
        e = self.engine
        if self._cur is None:
            self._cur = torch.empty((self.n, self.proj["proj_h"], self.proj["proj_w"]), dtype=torch.float32, device=e.device)
            self._valid = np.full(self.n, -1, np.int64)
        todo = np.unique(scans[self._valid[scans] < 0])
        if todo.size == 0:
            return self._cur, self._valid
        # runs of consecutive scans share a launch (at most 512 images of scratch); a subsampled list gives one scan per launch
        cuts = np.nonzero(np.diff(todo) != 1)[0] + 1
        for run in np.split(todo, cuts):
            for s0 in range(int(run[0]), int(run[-1]) + 1, 512):
                s1 = min(int(run[-1]) + 1, s0 + 512)
                off = (self._offsets[s0:s1 + 1] - self._offsets[s0]).contiguous()
                p0, p1 = int(self._host_offsets[s0]), int(self._host_offsets[s1])
                self._cur[s0:s1] = e.gt_range_images(self._points[p0:p1], off, self.max_points, **self.proj)
        idx = torch.from_numpy(todo).to(e.device)
        valid = [torch.count_nonzero(self._cur[idx[a:a + 512]] > 0, dim=(1, 2)) for a in range(0, len(todo), 512)]
        self._valid[todo] = torch.cat(valid).cpu().numpy()      # `valid_num` (com_overlap_yaw.py:32-33); the one sync here
        return self._cur, self._valid

    def _pair_counts(self, fr: np.ndarray, rf: Optional[np.ndarray], frames_per_pass: Optional[int]) -> np.ndarray:
        """(F, R) int64 counts of frames `fr` against scans `rf` (None = all): one launch and one synchronisation per pass."""
        e = self.engine
        cur, _ = self._own_ranges(fr)
        if self._inv_poses is None:                             # N host inversions, each the call `overlaps` makes
            inv = np.stack([np.linalg.inv(p) for p in self.poses]) if self.n else np.zeros((0, 4, 4))
            self._inv_poses = torch.from_numpy(np.ascontiguousarray(inv)).to(e.device)
        F, R = len(fr), self.n if rf is None else len(rf)
        if frames_per_pass is None:
            frames_per_pass = max(1, (64 << 20) // (4 * max(R, 1)))
        if frames_per_pass < 1:
            raise ValueError("frames_per_pass must be at least 1")
        ref_idx = None if rf is None else torch.from_numpy(rf.astype(np.int32)).to(e.device)
        counts = np.zeros((F, R), np.int64)
        for a in range(0, F, frames_per_pass):
            b = min(F, a + frames_per_pass)
            frame_idx = torch.from_numpy(fr[a:b].astype(np.int32)).to(e.device)
            c = e.gt_pair_counts(self._points, self._offsets, self._ref_poses, self._inv_poses, cur, frame_idx, ref_idx,
                                 fov_up=self.proj["fov_up"], fov_down=self.proj["fov_down"], max_range=self.proj["max_range"])
            counts[a:b] = c.cpu().numpy()
        return counts

    def all_pairs(self, frames: Optional[Sequence[int]] = None, refs: Optional[Sequence[int]] = None,
                  frames_per_pass: Optional[int] = None) -> dict:
        """Labels of every frame in `frames` against every scan in `refs` (None = all scans in order; lists may repeat and need
        not be sorted): {"overlaps": (F, R) float64, "yaw_bins": (F, R) int64, "valid": (F,) int64}.  overlaps[f, r] divides the
        same two integers as `overlaps(frames[f])[refs[r]]`; a frame without a point inside the field of view raises the same
        ZeroDivisionError.

        One kernel labels a pass of `frames_per_pass` frames against all refs without a range image per pair
        (csrc/overlap_gt.hip, gt_pair_kernel); the host synchronises once per pass.  Device footprint beside the resident scans:
        the own range images, n x H x W x 4 B and kept on the object (1.05 GB for the 4541 scans of KITTI 00 at 64 x 900, 254 MB
        for the 1101 of sequence 07), n inverse poses, and frames_per_pass x R x 4 B of counts per pass -- by default at most
        64 MB (3694 frames of sequence 00 per pass, two passes).  The yaw bins are host arithmetic (`yaw_bins_all`)."""
        fr = np.arange(self.n) if frames is None else np.asarray(frames, np.int64).reshape(-1)
        rf = np.arange(self.n) if refs is None else np.asarray(refs, np.int64).reshape(-1)
        for what, idx in (("frames", fr), ("refs", rf)):
            if idx.size and (idx.min() < 0 or idx.max() >= self.n):
                raise IndexError("%s must lie in [0, %d)" % (what, self.n))
        F, R = len(fr), len(rf)
        out = {"overlaps": np.zeros((F, R)), "yaw_bins": np.zeros((F, R), np.int64), "valid": np.zeros(F, np.int64)}
        if F == 0:
            return out
        cur, valid = self._own_ranges(fr)
        out["valid"] = valid[fr].copy()
        if R == 0:
            return out
        empty = np.nonzero(out["valid"] == 0)[0]
        if empty.size:
            raise ZeroDivisionError("frame %d has no point inside the field of view" % int(fr[empty[0]]))
        counts = self._pair_counts(fr, None if refs is None else rf, frames_per_pass)
        out["overlaps"] = counts / out["valid"][:, None].astype(np.float64)
        out["yaw_bins"] = yaw_bins_all(self.poses, fr, rf, self.leg_output_width)
        return out

    def mapping_all(self, frames: Optional[Sequence[int]] = None) -> np.ndarray:
        """(F * n, 4) rows [frame, ref, overlap, yaw_bin], frame-major: `mapping(f)` of every frame in `frames` (None = all),
        concatenated -- the reference's ground_truth_mapping for a whole sequence."""
        fr = np.arange(self.n) if frames is None else np.asarray(frames, np.int64).reshape(-1)
        lab = self.all_pairs(fr)
        m = np.zeros((len(fr) * self.n, 4))
        m[:, 0] = np.repeat(fr, self.n)
        m[:, 1] = np.tile(np.arange(self.n), len(fr))
        m[:, 2] = lab["overlaps"].reshape(-1)
        m[:, 3] = lab["yaw_bins"].reshape(-1)
        return m

    def mapping(self, frame_idx: int) -> np.ndarray:
        m = np.zeros((self.n, 4))
        m[:, 0] = np.ones(self.n) * frame_idx
        m[:, 1] = np.arange(self.n)
        m[:, 2] = self.overlaps(frame_idx)
        m[:, 3] = [yaw_bin(self.poses[frame_idx], self.poses[r], self.leg_output_width) for r in range(self.n)]
        return m


def com_overlap_yaw(scan_paths: List[str], poses, frame_idx: int, leg_output_width: int = 360,
                    engine: Optional[OvnEngine] = None) -> np.ndarray:
    """Same signature and result as the reference's com_overlap_yaw (com_overlap_yaw.py:10-68)."""
    print('Start to compute ground truth overlap and yaw ...')
    scans = [np.fromfile(p, dtype=np.float32).reshape((-1, 4)) for p in scan_paths]
    gt = OverlapGroundTruth(scans, np.asarray(poses), engine=engine, leg_output_width=leg_output_width)
    ground_truth_mapping = gt.mapping(frame_idx)
    print('Finish generating ground_truth_mapping!')
    return ground_truth_mapping
