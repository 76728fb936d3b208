"""Raw KITTI scans + poses -> the ground-truth files the trainer reads (the reference's demo/demo4_gen_gt_files.py without the
plot, for every frame of the sequence instead of frame 0):

    python tools/build_training_set.py --scans sequences/07/velodyne --poses poses/07.txt --calib sequences/07/calib.txt \\
        --dst out/07 --seq 07 [--frames every 5] [--proj-h 32 --proj-w 900 --fov-up 10.67 --fov-down -30.67 --max-range 50]

writes out/07/ground_truth/{train_set,validation_set,ground_truth_overlap_yaw}.npz (`overlaps` (n,4) rows
[frame, ref, overlap, yaw_bin] + `seq`), which `OverlapNetTrainer.fit_from_npz` and `evaluate.run_test` read.  The poses file
holds one camera pose per line (12 numbers, a 3 x 4 matrix); they are moved into the LiDAR frame of the first scan with the
calibration's `Tr:` line, as demo4_gen_gt_files.py:61-74 does.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _homogeneous(numbers) -> np.ndarray:
    m = np.eye(4)
    m[:3, :] = np.asarray(numbers, np.float64).reshape(3, 4)
    return m


def read_poses(path: str) -> np.ndarray:
    """(n,4,4) camera poses: a KITTI odometry text file, or an npz whose first array holds them."""
    if path.endswith(".txt"):
        with open(path) as f:
            return np.stack([_homogeneous(line.split()) for line in f if line.strip()])
    with np.load(path) as z:
        return np.asarray(z[z.files[0]], np.float64).reshape(-1, 4, 4)


def read_calib(path: str) -> np.ndarray:
    """T_cam_velo (4,4) from the `Tr:` line of a KITTI calib.txt."""
    with open(path) as f:
        for line in f:
            if line.startswith("Tr:"):
                return _homogeneous(line[3:].split())
    raise ValueError("%s has no 'Tr:' line" % path)


def lidar_poses(cam_poses: np.ndarray, t_cam_velo: np.ndarray) -> np.ndarray:
    """Camera poses -> LiDAR poses relative to the first frame: T_velo_cam . inv(pose_0) . pose . T_cam_velo."""
    t_velo_cam = np.linalg.inv(t_cam_velo)
    pose0_inv = np.linalg.inv(cam_poses[0])
    return np.stack([t_velo_cam.dot(pose0_inv).dot(p).dot(t_cam_velo) for p in cam_poses])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", required=True, help="folder of .bin scans (sorted by name = frame order)")
    ap.add_argument("--poses", required=True)
    ap.add_argument("--calib", required=True)
    ap.add_argument("--dst", required=True)
    ap.add_argument("--seq", required=True, help="sequence name stored beside every pair, e.g. 07")
    ap.add_argument("--frames", nargs=2, metavar=("every", "K"), default=None,
                    help="label only every K-th scan as a current frame (against all scans)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--proj-h", type=int, default=64)
    ap.add_argument("--proj-w", type=int, default=900)
    ap.add_argument("--fov-up", type=float, default=3.0)
    ap.add_argument("--fov-down", type=float, default=-25.0)
    ap.add_argument("--max-range", type=float, default=50.0)
    ap.add_argument("--leg-output-width", type=int, default=360, help="number of yaw bins")
    a = ap.parse_args()
    if a.frames is not None and (a.frames[0] != "every" or not a.frames[1].isdigit() or int(a.frames[1]) < 1):
        ap.error("--frames takes `every K` with K >= 1")

    from overlapnet_amd.dataset import build_training_set
    paths = sorted(os.path.join(dp, f) for dp, _, fn in os.walk(os.path.expanduser(a.scans)) for f in fn)
    poses = lidar_poses(read_poses(a.poses), read_calib(a.calib))
    if len(paths) != len(poses):
        raise SystemExit("%d scans in %s but %d poses in %s" % (len(paths), a.scans, len(poses), a.poses))
    frames = None if a.frames is None else range(0, len(paths), int(a.frames[1]))
    t0 = time.perf_counter()
    mapping, train, val = build_training_set(paths, poses, a.dst, a.seq, frames=frames, seed=a.seed, proj_H=a.proj_h,
                                             proj_W=a.proj_w, fov_up=a.fov_up, fov_down=a.fov_down, max_range=a.max_range,
                                             leg_output_width=a.leg_output_width)
    print(json.dumps({"tool": "tools/build_training_set.py", "scans": len(paths), "pairs": len(mapping), "train": len(train),
                      "validation": len(val), "seconds": round(time.perf_counter() - t0, 3),
                      "folder": os.path.join(a.dst, "ground_truth")}))


if __name__ == "__main__":
    main()
