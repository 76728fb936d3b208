"""GPU: whole-sequence labelling -- `ovn_gt_pair_counts` (csrc/overlap_gt.hip, gt_pair_kernel), `OverlapGroundTruth.all_pairs` /
`mapping_all` and `dataset.build_training_set`.  Every equality is exact: the counts are integers, and the pair kernel and the
range-image path share one projection function."""
import os

import numpy as np
import pytest
import torch

import _gt_pairs_ref as R

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
SMALL = [dict(proj_H=5, proj_W=37), dict(proj_H=16, proj_W=45)]


@pytest.fixture(scope="module")
def golden(fixture_npz):
    z = np.load(os.path.join(G, "gt_overlap_yaw.npz"))
    return z, [fixture_npz["points_%d" % s] for s in z["scan_of"]]


@pytest.fixture(scope="module")
def gt_full(golden):
    """The 15 golden scans resident at 64 x 900, and `all_pairs()` of them, computed once."""
    from overlapnet_amd.ground_truth import OverlapGroundTruth
    z, scans = golden
    gt = OverlapGroundTruth(scans, z["poses"])
    return gt, gt.all_pairs()


def _pair_counts_by_images(gt, frame):
    """Counts of `frame` against every scan the range-image way (gt_range_images + gt_overlap_counts), and valid_num."""
    e = gt.engine
    off = gt._offsets.cpu().numpy()
    lo, hi = int(off[frame]), int(off[frame + 1])
    one = torch.tensor([0, hi - lo], dtype=torch.int64, device=e.device)
    cur = e.gt_range_images(gt._points[lo:hi], one, hi - lo, **gt.proj)
    inv = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(gt.poses[frame]))).to(e.device)
    imgs = e.gt_range_images(gt._points, gt._offsets, gt.max_points, gt._ref_poses, inv, **gt.proj)
    c = e.gt_overlap_counts(imgs, cur).cpu().numpy()
    return c[:-1], int(c[-1])


def test_all_pairs_equals_overlaps_and_golden(golden, gt_full):
    z, _ = golden
    gt, lab = gt_full
    n = gt.n
    assert lab["overlaps"].shape == (n, n) and lab["overlaps"].dtype == np.float64
    assert lab["yaw_bins"].shape == (n, n) and lab["yaw_bins"].dtype == np.int64
    assert lab["valid"].shape == (n,) and lab["valid"].dtype == np.int64
    for f in range(n):
        assert np.array_equal(lab["overlaps"][f], gt.overlaps(f)), f
    assert np.array_equal(np.diag(lab["overlaps"]), np.ones(n))
    rows = gt.mapping_all()
    assert rows.shape == (n * n, 4)
    for f in (0, 4, 7, 11):
        assert np.array_equal(rows[f * n:(f + 1) * n], z["mapping_%d" % f]), f
    sub = gt.mapping_all([11, 4])
    assert np.array_equal(sub, np.concatenate([z["mapping_11"], z["mapping_4"]]))


def test_index_lists_passes_and_repeat_calls(gt_full):
    gt, lab = gt_full
    frames, refs = [9, 2, 14, 2, 0], [13, 1, 1, 7, 0, 5, 12]
    part = gt.all_pairs(frames, refs)
    for key in ("overlaps", "yaw_bins"):
        assert np.array_equal(part[key], lab[key][np.ix_(frames, refs)]), key
    assert np.array_equal(part["valid"], lab["valid"][frames])
    only_frames = gt.all_pairs(frames=frames)
    assert np.array_equal(only_frames["overlaps"], lab["overlaps"][frames])
    only_refs = gt.all_pairs(refs=refs)
    assert np.array_equal(only_refs["overlaps"], lab["overlaps"][:, refs])
    for fpp in (1, 4, None):
        again = gt.all_pairs(frames_per_pass=fpp)
        for key in lab:
            assert np.array_equal(again[key], lab[key]), (fpp, key)
    empty = gt.all_pairs(frames=[], refs=[3])
    assert empty["overlaps"].shape == (0, 1)


@pytest.mark.parametrize("geometry", SMALL, ids=["5x37", "16x45"])
def test_pair_counts_equal_range_image_counts_on_ragged_scans(fixture_npz, geometry):
    """An empty scan, one point, 257 points, (0,0,0) and points beyond max_range; 185 and 720 pixels (partial last word /
    whole words).  Frame by frame the kernel's integers against gt_overlap_counts', and against the host restatement."""
    from overlapnet_amd.ground_truth import OverlapGroundTruth
    scans, poses = R.ragged_scans(fixture_npz)
    gt = OverlapGroundTruth(scans, poses, **geometry)
    e = gt.engine
    cur, valid = gt._own_ranges(np.arange(gt.n))
    inv = torch.from_numpy(np.stack([np.linalg.inv(p) for p in poses])).to(e.device)
    counts = e.gt_pair_counts(gt._points, gt._offsets, gt._ref_poses, inv, cur, fov_up=gt.proj["fov_up"],
                              fov_down=gt.proj["fov_down"], max_range=gt.proj["max_range"]).cpu().numpy()
    assert counts.shape == (gt.n, gt.n) and counts.dtype == np.int32
    for f in range(gt.n):
        by_images, v = _pair_counts_by_images(gt, f)
        assert np.array_equal(counts[f], by_images), (f, counts[f], by_images)
        assert valid[f] == v
        host, _, host_valid = R.pair_counts(scans, poses, f, **geometry)
        assert np.array_equal(counts[f], host) and v == host_valid, (f, counts[f], host)
    assert valid[1] == 0 and np.all(counts[:, 1] == 0) and np.all(counts[1] == 0)       # the empty scan
    assert counts.max() > 0
    # index lists straight into the entry point: unsorted, with a repeat
    fi = torch.tensor([4, 0, 4], dtype=torch.int32, device=e.device)
    ri = torch.tensor([5, 5, 2, 0], dtype=torch.int32, device=e.device)
    sub = e.gt_pair_counts(gt._points, gt._offsets, gt._ref_poses, inv, cur, fi, ri, fov_up=gt.proj["fov_up"],
                           fov_down=gt.proj["fov_down"], max_range=gt.proj["max_range"]).cpu().numpy()
    assert np.array_equal(sub, counts[np.ix_([4, 0, 4], [5, 5, 2, 0])])
    # a frame whose scan is empty cannot be a current frame; the others still can
    with pytest.raises(ZeroDivisionError, match="frame 1 "):
        gt.all_pairs()
    ok = [0, 2, 3, 4, 5]
    lab = gt.all_pairs(frames=ok)
    assert np.array_equal(lab["overlaps"], counts[ok] / valid[ok][:, None])


def test_three_points_on_one_ray_gpu():
    from overlapnet_amd.ground_truth import OverlapGroundTruth
    scans, poses, expect = R.ray_scans()
    gt = OverlapGroundTruth(scans, poses)
    lab = gt.all_pairs(frames=[0])
    assert lab["valid"][0] == 1
    assert np.array_equal(lab["overlaps"][0], expect.astype(np.float64))       # scan 1 hits AND is blocked: 0
    assert np.array_equal(lab["overlaps"][0], gt.overlaps(0))


def _tiny_inputs(e, h, w):
    pts = np.zeros((100, 4), np.float32)
    pts[:, 0] = np.linspace(2.0, 30.0, 100)
    pts[:, 1] = np.linspace(-5.0, 9.0, 100)
    pts[:, 2] = np.linspace(-1.5, 0.2, 100)
    points = torch.from_numpy(np.concatenate([pts, pts[::-1]])).to(e.device)
    offsets = torch.tensor([0, 100, 200], dtype=torch.int64, device=e.device)
    poses = torch.from_numpy(np.stack([np.eye(4)] * 2)).to(e.device)
    cur = e.gt_range_images(points, offsets, 100, proj_h=h, proj_w=w)
    return points, offsets, poses, cur


def test_lds_limit_accepted_and_refused():
    """H * W = 262,144 fills the 64 KB of LDS exactly and runs; 262,176 is one word per plane more: refused, nothing launched."""
    from overlapnet_amd import _lib
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 1)
    points, offsets, poses, cur = _tiny_inputs(e, 512, 512)
    counts = e.gt_pair_counts(points, offsets, poses, poses, cur).cpu().numpy()
    valid = torch.count_nonzero(cur > 0, dim=(1, 2)).cpu().numpy()
    assert valid[0] > 50
    assert np.array_equal(counts, np.array([[valid[0], valid[0]], [valid[1], valid[1]]]))   # both scans hold the same points
    big = torch.zeros((2, 1, 262176), dtype=torch.float32, device=e.device)
    torch.cuda.synchronize()
    with pytest.raises(_lib.OvnError, match="LDS"):
        e.gt_pair_counts(points, offsets, poses, poses, big)
    torch.cuda.synchronize()                                                   # no launch happened, so no late error either
    with pytest.raises(_lib.OvnError, match="contiguous"):
        e.gt_pair_counts(points, offsets, poses.float(), poses, cur)
    e.close()


def test_pair_index_past_one_launch():
    """3000 x 3000 pairs by index lists over 3 tiny scans: more workgroups than one launch carries (2^23), so the pair index
    continues in a second launch; every pair equals its entry of the 3 x 3 table."""
    from overlapnet_amd.ground_truth import OverlapGroundTruth
    scans = [np.array([[5, 0, 0, 0], [0, 7, -1, 0]], np.float32), np.array([[5.5, 0, 0, 0]], np.float32),
             np.array([[0, 7.2, -1, 0], [20, 20, 0, 0], [5.2, 0, 0, 0]], np.float32)]
    gt = OverlapGroundTruth(scans, np.stack([np.eye(4)] * 3), proj_H=4, proj_W=16)
    e = gt.engine
    cur, _ = gt._own_ranges(np.arange(3))
    geometry = dict(fov_up=gt.proj["fov_up"], fov_down=gt.proj["fov_down"], max_range=gt.proj["max_range"])
    table = e.gt_pair_counts(gt._points, gt._offsets, gt._ref_poses, gt._ref_poses, cur, **geometry).cpu().numpy()
    assert len(np.unique(table)) > 1
    rng = np.random.default_rng(0)
    frames, refs = rng.integers(0, 3, 3000).astype(np.int32), rng.integers(0, 3, 3000).astype(np.int32)
    big = e.gt_pair_counts(gt._points, gt._offsets, gt._ref_poses, gt._ref_poses, cur, torch.from_numpy(frames).to(e.device),
                           torch.from_numpy(refs).to(e.device), **geometry).cpu().numpy()
    assert big.shape == (3000, 3000)
    assert np.array_equal(big, table[np.ix_(frames, refs)])


def test_build_training_set_writes_what_the_trainer_reads(golden, tmp_path):
    from overlapnet_amd.dataset import build_training_set
    from overlapnet_amd.evaluate import load_pairs
    z, scans = golden
    paths = []
    for i, s in enumerate(scans):
        paths.append(str(tmp_path / ("%06d.bin" % i)))
        np.ascontiguousarray(s, np.float32).tofile(paths[-1])
    mapping, train, val = build_training_set(paths, z["poses"], str(tmp_path), "07", seed=0)
    n = len(scans)
    assert mapping.shape == (n * n, 4)
    for f in (0, 4, 7, 11):
        assert np.array_equal(mapping[f * n:(f + 1) * n], z["mapping_%d" % f])
    assert len(val) == (len(train) + len(val)) // 10
    folder = tmp_path / "ground_truth"
    for name, rows in (("train_set", train), ("validation_set", val), ("ground_truth_overlap_yaw", mapping)):
        f1, f2, d1, d2, ov, yaw = load_pairs([str(folder / (name + ".npz"))])
        assert f1 == ["%06d" % v for v in rows[:, 0]] and f2 == ["%06d" % v for v in rows[:, 1]]
        assert set(d1) | set(d2) == {"07"}
        assert np.array_equal(ov, rows[:, 2]) and np.array_equal(yaw, rows[:, 3])
    m2, t2, v2 = build_training_set(paths, z["poses"], str(tmp_path), "07", seed=0)
    assert np.array_equal(t2, train) and np.array_equal(v2, val)
    sub, _, _ = build_training_set(paths, z["poses"], str(tmp_path), "07", frames=range(0, n, 4), seed=0)
    assert np.array_equal(sub, mapping.reshape(n, n, 4)[::4].reshape(-1, 4))
