"""CPU: the host half of whole-sequence labelling -- the two-flag overlap count the pair kernel implements (restated in
tests/_gt_pairs_ref.py) against the range-image count, `yaw_bins_all` against the scalar `yaw_bin`, and the dataset builder's
normalise / split / write steps."""
import os

import numpy as np
import pytest

import _gt_pairs_ref as R
from oracle import overlapnet_oracle as O
from overlapnet_amd import dataset as D
from overlapnet_amd.evaluate import load_pairs
from overlapnet_amd.ground_truth import yaw_bin, yaw_bins_all

G = os.path.join(os.path.dirname(__file__), "golden")
FRAMES = (0, 4, 7, 11)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(G, "gt_overlap_yaw.npz"))
    pts = np.load(os.path.join(G, "kitti_preprocess.npz"))
    fixture = {"points_0": pts["points_0"], "points_1": pts["points_1"]}
    return z, [fixture["points_%d" % s] for s in z["scan_of"]], fixture


# ---- the two-flag count ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES)
def test_two_flag_count_equals_oracle_on_golden_pairs(golden, frame):
    z, scans, _ = golden
    poses = z["poses"]
    cur = O.range_image_f64(R.homog(scans[frame]))
    valid = int(np.count_nonzero(cur > 0))
    inv_cur = np.linalg.inv(poses[frame])
    ov = np.array([R.two_flag_count(*R.project(R.moved(scans[r], poses[r], inv_cur)), cur.reshape(-1)) / valid
                   for r in range(len(scans))])
    assert np.array_equal(ov, O.com_overlap_yaw(scans, poses, frame)[:, 2])
    assert np.array_equal(ov, z["mapping_%d" % frame][:, 2])                     # and the reference's own numbers


def test_two_flag_count_small_geometry_partial_word(golden):
    """185 pixels: the last 32-bit word of a plane holds 25; many points per pixel, so nearer points block often."""
    z, scans, _ = golden
    scans = [s[:3000] for s in scans]
    blocked_some = False
    for frame in FRAMES:
        flags, images, valid = R.pair_counts(scans, z["poses"], frame, proj_H=5, proj_W=37)
        assert valid > 0
        assert np.array_equal(flags, images), (frame, flags, images)
        blocked_some |= bool(np.any(images < valid))
    assert blocked_some


def test_three_points_on_one_ray():
    scans, poses, expect = R.ray_scans()
    pix = [R.project(R.homog(s))[0] for s in scans]
    assert len({int(p) for a in pix for p in a}) == 1                           # all on one pixel, or the case tests nothing
    flags, images, valid = R.pair_counts(scans, poses, 0)
    assert valid == 1
    assert np.array_equal(images, expect)
    assert np.array_equal(flags, expect)                                        # scan 1: hit AND blocked -> does not count


# ---- yaw bins ----------------------------------------------------------------------------------------------------------
def _scalar_bins(poses, frames, refs, w=360):
    return np.array([[yaw_bin(poses[f], poses[r], w) for r in refs] for f in frames], np.int64)


def test_yaw_bins_all_golden_poses(golden):
    z, _, _ = golden
    poses = z["poses"]
    n = len(poses)
    got = yaw_bins_all(poses)
    assert got.shape == (n, n) and got.dtype == np.int64
    assert np.array_equal(got, _scalar_bins(poses, range(n), range(n)))
    for f in FRAMES:
        assert np.array_equal(got[f], z["mapping_%d" % f][:, 3])
    # index lists, unsorted with a repeat, and another resolution
    fr, rf = [7, 2, 7, 14], [3, 0, 11, 3, 8]
    assert np.array_equal(yaw_bins_all(poses, fr, rf, 90), _scalar_bins(poses, fr, rf, 90))


def test_yaw_bins_all_pure_translation_pairs():
    poses = R.translation_pairs(2000, seed=0)
    scalar = np.array([yaw_bin(poses[2 * k], poses[2 * k + 1]) for k in range(2000)])
    assert set(np.unique(scalar)) == {179, 180}                                  # rounding noise decides: the boundary IS hit
    got = np.array([yaw_bins_all(poses, [2 * k], [2 * k + 1])[0, 0] for k in range(2000)])
    assert np.array_equal(got, scalar)
    # and as blocks, where the vectorised path sees many references per frame
    for a in range(0, 4000, 400):
        idx = np.arange(a, a + 400)
        assert np.array_equal(yaw_bins_all(poses, idx[::40], idx), _scalar_bins(poses, idx[::40], idx))


def test_yaw_bins_all_identical_and_gimbal_poses():
    eye = np.stack([np.eye(4)] * 3)
    assert np.array_equal(yaw_bins_all(eye), np.full((3, 3), 180))
    assert np.array_equal(yaw_bins_all(eye), _scalar_bins(eye, range(3), range(3)))
    # pitch of +-90 degrees against level poses: R[2,0] = -+1, the scalar function leaves the yaw at 0
    poses = [np.eye(4)]
    for pitch in (np.pi / 2, -np.pi / 2, np.pi / 2 - 3e-6, np.pi / 2 - 3e-5, 1.0):
        T = np.eye(4)
        T[:3, :3] = [[np.cos(pitch), 0, np.sin(pitch)], [0, 1, 0], [-np.sin(pitch), 0, np.cos(pitch)]]
        yaw = 0.7
        Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]])
        T[:3, :3] = Rz @ T[:3, :3]
        poses.append(T)
    poses = np.stack(poses)
    n = len(poses)
    assert np.array_equal(yaw_bins_all(poses), _scalar_bins(poses, range(n), range(n)))
    assert yaw_bins_all(poses, [], [0, 1]).shape == (0, 2)


# ---- dataset builder ---------------------------------------------------------------------------------------------------
def _mapping(sizes, seed=5):
    """Rows with sizes[k] overlaps inside bin k, shuffled; columns 0/1 number the rows so that they can be told apart."""
    rng = np.random.default_rng(seed)
    ov = np.concatenate([rng.uniform(0.1 * k + 0.001, 0.1 * k + 0.099, s) for k, s in enumerate(sizes)])
    m = np.zeros((len(ov), 4))
    m[:, 0] = np.arange(len(ov))
    m[:, 1] = np.arange(len(ov))[::-1]
    m[:, 2] = ov
    m[:, 3] = rng.integers(0, 361, len(ov))
    return m[rng.permutation(len(ov))]


def _bin_of(ov):
    return np.minimum((ov * 10).astype(int), 9)


def test_normalize_overlaps_bin_sizes_and_seed():
    sizes = [500, 40, 3, 17, 25, 8, 0, 30, 2, 60]
    m = _mapping(sizes)
    m[np.nonzero(_bin_of(m[:, 2]) == 9)[0][0], 2] = 1.0                          # overlap 1 belongs to the last bin
    out = D.normalize_overlaps(m, np.random.default_rng(3))
    got = np.bincount(_bin_of(out[:, 2]), minlength=10)
    assert list(got) == [25, 25, 25, 25, 25, 8, 0, 30, 2, 60]
    assert np.all(np.diff(_bin_of(out[:, 2])) >= 0)                              # concatenated in bin order
    rows = {tuple(r) for r in m}
    assert all(tuple(r) in rows for r in out)                                    # rows are taken whole
    for k in (5, 7, 8, 9):                                                        # kept whole and in their original order
        assert np.array_equal(out[_bin_of(out[:, 2]) == k], m[_bin_of(m[:, 2]) == k])
    assert len({tuple(r) for r in out[_bin_of(out[:, 2]) == 2]}) <= 3           # 3 rows resampled to 25: with replacement
    assert np.array_equal(out, D.normalize_overlaps(m, np.random.default_rng(3)))
    assert not np.array_equal(out, D.normalize_overlaps(m, np.random.default_rng(4)))


def test_normalize_overlaps_empty_bins():
    out = D.normalize_overlaps(_mapping([50, 0, 0, 9, 4, 3, 0, 0, 0, 5]), np.random.default_rng(0))
    assert list(np.bincount(_bin_of(out[:, 2]), minlength=10)) == [4, 0, 0, 4, 4, 3, 0, 0, 0, 5]
    with pytest.raises(ValueError, match=r"\[0\.4, 0\.5\)"):
        D.normalize_overlaps(_mapping([50, 5, 5, 5, 0, 3, 1, 1, 1, 5]), np.random.default_rng(0))


@pytest.mark.parametrize("n", [0, 9, 10, 137])
def test_split_train_val(n):
    m = _mapping([n, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    train, val = D.split_train_val(m, np.random.default_rng(1))
    assert len(val) == n // 10 and len(train) == n - n // 10
    ids = np.concatenate([train[:, 0], val[:, 0]])
    assert np.array_equal(np.sort(ids), np.arange(n))                            # disjoint and complete
    both = np.concatenate([train, val])
    assert np.array_equal(both[np.argsort(both[:, 0])], m[np.argsort(m[:, 0])])
    t2, v2 = D.split_train_val(m, np.random.default_rng(1))
    assert np.array_equal(train, t2) and np.array_equal(val, v2)


def test_write_ground_truth_round_trip(tmp_path):
    m = _mapping([30, 6, 6, 6, 6, 4, 4, 4, 4, 10])
    rng = np.random.default_rng(2)
    train, val = D.split_train_val(D.normalize_overlaps(m, rng), rng)
    folder = D.write_ground_truth(str(tmp_path), "07", m, train, val)
    assert folder == os.path.join(str(tmp_path), "ground_truth")
    for name, rows in (("train_set", train), ("validation_set", val), ("ground_truth_overlap_yaw", m)):
        f1, f2, d1, d2, ov, yaw = load_pairs([os.path.join(folder, name + ".npz")])
        assert f1 == ["%06d" % v for v in rows[:, 0]] and f2 == ["%06d" % v for v in rows[:, 1]]
        assert d1 == ["07"] * len(rows) and d2 == ["07"] * len(rows)
        assert np.array_equal(ov, rows[:, 2]) and np.array_equal(yaw, rows[:, 3])
        with np.load(os.path.join(folder, name + ".npz"), allow_pickle=True) as h:
            assert sorted(h.files) == ["overlaps", "seq"] and h["seq"].shape == (len(rows), 2) and h["seq"].dtype == object
    D.write_ground_truth(str(tmp_path), "07", m, train, val)                     # an existing folder is written into again


# ---- the command-line tool's pose handling and the entry point's argument checks ------------------------------------------
def test_tool_reads_kitti_poses_and_calib(tmp_path):
    from tools import build_training_set as T
    rng = np.random.default_rng(0)
    cam = np.stack([np.eye(4)] * 3)
    cam[:, :3, :] = rng.normal(size=(3, 3, 4))
    tr = np.eye(4)
    tr[:3, :] = rng.normal(size=(3, 4))
    (tmp_path / "poses.txt").write_text("".join(" ".join(repr(float(v)) for v in p[:3].reshape(-1)) + "\n" for p in cam))
    (tmp_path / "calib.txt").write_text("P0: 1 0 0 0 0 1 0 0 0 0 1 0\nTr: " + " ".join(repr(float(v)) for v in tr[:3].reshape(-1)) + "\n")
    poses, calib = T.read_poses(str(tmp_path / "poses.txt")), T.read_calib(str(tmp_path / "calib.txt"))
    assert np.array_equal(poses, cam) and np.array_equal(calib, tr)
    out = T.lidar_poses(poses, calib)
    expect = [np.linalg.inv(tr).dot(np.linalg.inv(cam[0])).dot(p).dot(tr) for p in cam]
    assert np.array_equal(out, np.stack(expect))
    assert np.allclose(out[0], np.eye(4), atol=1e-9)              # the first scan's LiDAR frame is the origin
    (tmp_path / "nocalib.txt").write_text("P0: 1 0 0 0\n")
    with pytest.raises(ValueError, match="Tr:"):
        T.read_calib(str(tmp_path / "nocalib.txt"))


def test_pair_counts_entry_rejects_null_context_before_any_gpu_call():
    from overlapnet_amd import _lib
    lib = _lib.load()
    assert lib.ovn_gt_pair_counts(None, None, None, 0, None, None, None, None, 0, None, 0, 64, 900, 3.0, -25.0, 50.0, None, None) == 1
    assert b"ovn_gt_pair_counts: ctx is NULL" in lib.ovn_last_error()
