"""From raw scans and poses to the files the trainer reads -- the second half of the reference's demo4_gen_gt_files.py.

`build_training_set` labels every requested frame of a sequence against every scan on the GPU
(`OverlapGroundTruth.mapping_all`), balances the overlap distribution (src/utils/normalize_data.py:17-45), splits off a tenth
for validation (src/utils/split_train_val.py:19-22) and writes `ground_truth/{train_set,validation_set,
ground_truth_overlap_yaw}.npz` in the `overlaps` + `seq` layout (demo4_gen_gt_files.py:96-109) that `evaluate.load_pairs` and
`OverlapNetTrainer.fit_from_npz` read.  Every random choice takes an explicit `numpy.random.Generator`.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import numpy as np

from .ground_truth import OverlapGroundTruth

N_OVERLAP_BINS = 10
BALANCE_BIN = 4          # the bin [0.4, 0.5) sets the size bins 0..4 are resampled to


def _overlap_bins(overlap: np.ndarray):
    """Boolean masks of the ten bins [0, .1), [.1, .2) ... [.8, .9), [.9, 1] (normalize_data.py:17-26; the first has no lower
    bound there, the last includes 1)."""
    edges =[0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]       # the reference's literals, not 0.1 * k (0.1 * 3 != 0.3)
    masks = [overlap < edges[0]]
    for k in range(1, N_OVERLAP_BINS - 1):
        masks.append((overlap < edges[k]) & (overlap >= edges[k - 1]))
    masks.append((overlap <= 1) & (overlap >= edges[-1]))
    return masks


def normalize_overlaps(mapping: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """Balance the overlap distribution of (n,4) rows [frame, ref, overlap, yaw_bin]: the five bins below 0.5 are resampled WITH
    replacement to the size of the bin [0.4, 0.5), the five from 0.5 up are kept whole, concatenated in bin order.  Where the
    reference would crash: an empty bin below 0.4 contributes nothing; an empty [0.4, 0.5) bin is an error, because it would
    silently remove every pair below 0.5."""
    mapping = np.asarray(mapping)
    bins = [mapping[m] for m in _overlap_bins(mapping[:, 2])]
    target = len(bins[BALANCE_BIN])
    if target == 0:
        raise ValueError("no pair with an overlap in [0.4, 0.5): that bin sets the size of every bin below 0.5, so the set cannot "
                         "be balanced (bin sizes: %s)" % [len(b) for b in bins])
    parts = []
    for k, b in enumerate(bins):
        if k <= BALANCE_BIN:
            if len(b):
                parts.append(b[rng.choice(len(b), target)])
        else:
            parts.append(b)
    return np.concatenate(parts)


def split_train_val(mapping: np.ndarray, rng: np.random.Generator) -> Tuple[np.ndarray, np.ndarray]:
    """(train, validation): validation = len // 10 rows of a random permutation, training = the rest, both in permuted order
    (what scikit-learn's train_test_split(test_size=int(len / 10)) does in split_train_val.py:19-22)."""
    mapping = np.asarray(mapping)
    perm = rng.permutation(len(mapping))
    n_val = len(mapping) // 10
    return mapping[perm[n_val:]], mapping[perm[:n_val]]


def write_ground_truth(dst_folder: str, seq: str, mapping: np.ndarray, train: np.ndarray, validation: np.ndarray) -> str:
    """Write the three files of demo4_gen_gt_files.py:96-109 into `dst_folder`/ground_truth and return that folder: each holds
    `overlaps` (n,4) and `seq` (n,2) object array filled with the sequence name."""
    out = os.path.join(dst_folder, "ground_truth")
    os.makedirs(out, exist_ok=True)
    for name, rows in (("train_set", train), ("validation_set", validation), ("ground_truth_overlap_yaw", mapping)):
        rows = np.asarray(rows)
        names = np.empty((rows.shape[0], 2), dtype=object)
        names[:] = seq
        np.savez_compressed(os.path.join(out, name), overlaps=rows, seq=names)
    return out


def build_training_set(scan_paths: Sequence[str], poses: np.ndarray, dst_folder: str, seq: str,
                       frames: Optional[Sequence[int]] = None, seed: int = 0, **geometry
                       ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Raw scans + poses -> `dst_folder`/ground_truth/*.npz; returns (mapping, train, validation).

    scan_paths: KITTI .bin files (float32 x, y, z, intensity), one per pose, in frame order; poses (n,4,4) in the LiDAR frame.
    frames: the current frames to label against all scans (None = every scan).  geometry: `OverlapGroundTruth`'s keywords
    (proj_H, proj_W, fov_up, fov_down, max_range, leg_output_width, engine) for a sensor other than the 64-beam default."""
    scans = [np.fromfile(p, dtype=np.float32).reshape((-1, 4)) for p in scan_paths]
    gt = OverlapGroundTruth(scans, np.asarray(poses), **geometry)
    mapping = gt.mapping_all(frames)
    rng = np.random.default_rng(seed)
    train, validation = split_train_val(normalize_overlaps(mapping, rng), rng)
    write_ground_truth(dst_folder, seq, mapping, train, validation)
    return mapping, train, validation
