"""CPU: the fp64 NumPy reference of the range-image ICP (tests/_icp_ref.py) converges on the fixtures the GPU tests use, the yaw-bin
convention of `registration.pose_from_yaw_bin` is the ground-truth generator's, and the C ABI declares and binds `ovn_icp_register`."""
import os
import re

import numpy as np
import pytest

import _icp_ref as R
from oracle import overlapnet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _maps(cloud, H=64, W=900):
    rng, vtx, _, _ = O.range_projection(cloud, proj_H=H, proj_W=W)
    return rng, vtx, O.gen_normal_map(rng, vtx, H, W)


@pytest.fixture(scope="module")
def target_maps(fixture_npz):
    return _maps(fixture_npz["points_0"])


# per case: the largest translation [m] / rotation [deg] error the reference may end with (measured: 0.8 / 1.7 / 1.7 / 4.6 mm and
# 0.006 / 0.003 / 0.003 / 0.005 deg, 16-28 k inliers)
@pytest.mark.parametrize("case, max_t", list(zip(R.REAL_CASES, (1.0e-3, 2.0e-3, 2.0e-3, 5.0e-3))))
def test_reference_recovers_a_moved_real_scan(fixture_npz, target_maps, case, max_t):
    yaw, t, off = case
    T_gt = R.make_pose(yaw, t)
    src = _maps(R.moved_cloud(fixture_npz["points_0"], np.linalg.inv(T_gt)))
    res = R.register(src, target_maps, R.rz(yaw + off))
    dt, dr = R.pose_error(res["pose"], T_gt)
    print(case, "error %.2f mm %.4f deg, %d inliers, rms %.4f" % (1e3 * dt, dr, res["inliers"], res["rms"]))
    assert res["status"] == 0 and res["solved"] == 20
    assert dt <= max_t and dr <= 0.01
    assert 16000 <= res["inliers"] <= 28000


def test_reference_registers_the_second_fixture_scan(fixture_npz, target_maps):
    res = R.register(_maps(fixture_npz["points_1"]), target_maps, np.eye(4))
    print(res["pose"][:3, 3], res["inliers"], res["rms"])
    assert res["status"] == 0
    assert abs(res["pose"][0, 3] - 0.68) < 0.01 and abs(res["pose"][1, 3]) < 0.02 and abs(res["pose"][2, 3]) < 0.02
    assert abs(res["inliers"] - 24330) <= 5 and abs(res["rms"] - 0.027) < 1e-3


@pytest.mark.parametrize("shape, max_t, inliers", [((16, 100), 3e-3, (1300, 1420)), ((8, 90), 2.5e-2, (530, 580)),
                                                   (R.ODD_ROOM_SHAPE, 5e-3, (1800, 2010))])
@pytest.mark.parametrize("case", R.ROOM_CASES)
def test_reference_converges_in_the_box_room(shape, max_t, inliers, case):
    H, W = shape
    tc, sc, T_gt, T0 = R.room_pair(case)
    res = R.register(_maps(sc, H, W), _maps(tc, H, W), T0)
    dt, dr = R.pose_error(res["pose"], T_gt)
    print(shape, case, "error %.2f mm %.4f deg, %d inliers of %d" % (1e3 * dt, dr, res["inliers"], res["valid"]))
    assert res["status"] == 0 and dt <= max_t and inliers[0] <= res["inliers"] <= inliers[1]


def test_degenerate_inputs_stop_the_reference():
    rng = np.full((8, 90), -1, np.float32)
    empty = (rng, np.full((8, 90, 4), -1, np.float32), np.full((8, 90, 3), -1, np.float32))
    T0 = R.make_pose(12.0, (0.1, 0.2, 0.3))
    res = R.register(empty, empty, T0)
    assert res["status"] == 1 and res["solved"] == 0 and np.array_equal(res["pose"], T0) and res["rms"] == 0.0


def test_se3_exp_is_a_rigid_motion_and_continuous_at_zero():
    g = np.random.default_rng(0)
    for scale in (1e-9, 0.9e-4, 1.1e-4, 0.3, 2.0):
        xi = g.normal(size=6) * scale
        T = R.se3_exp(xi)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14) and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-14
        # exp(xi) exp(-xi) = I
        assert np.allclose(T @ R.se3_exp(-xi), np.eye(4), atol=1e-14)


def test_pose_from_yaw_bin_follows_the_ground_truth_generator():
    """For every row [current, reference, overlap, yaw bin] the reference's com_overlap_yaw.py wrote: the angle of
    pose_from_yaw_bin(bin) is within one bin (1 degree) of the yaw of inv(pose_current) . pose_reference."""
    from overlapnet_amd.registration import pose_from_yaw_bin
    with np.load(os.path.join(G, "gt_overlap_yaw.npz")) as z:
        poses = z["poses"]
        rows = np.concatenate([z[k] for k in z.files if k.startswith("mapping_")])
    assert len(rows) == 60
    for cur, ref, _, b in rows:
        rel = np.linalg.inv(poses[int(cur)]) @ poses[int(ref)]
        yaw = np.degrees(np.arctan2(rel[1, 0], rel[0, 0]))
        T = pose_from_yaw_bin(b)
        assert T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1]) and np.array_equal(T[:3, 3], [0, 0, 0])
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-15) and T[2, 2] == 1.0
        phi = np.degrees(np.arctan2(T[1, 0], T[0, 0]))
        d = (phi - yaw + 180.0) % 360.0 - 180.0
        assert abs(d) <= 1.0 + 1e-9, (cur, ref, b, yaw, phi)
    # another bin count: width 180 has 2-degree bins
    assert np.allclose(pose_from_yaw_bin(45, 180)[:2, :2], [[0, -1], [1, 0]], atol=1e-15)


def test_pose_from_network_yaw_inverts_the_swapped_pair():
    """`Infer` returns yaw = 180 - argmax (evaluate.py inverts it as bin = 180 - yaw) for a pair whose FIRST leg is the reference and
    whose second is the current frame; the network is trained on [current, reference] rows to put its argmax at the row's bin.  So
    for the pair (reference r, current c) a perfect network's argmax is the bin of the ground-truth row [current = r, reference =
    c], and `pose_from_network_yaw` of the yaw `Infer` makes of it must be the rotation taking r's points into c's frame: within one
    bin of the yaw of inv(pose_c) . pose_r (the tilted frame 4 adds < 0.05 degrees: yaw(T^-1) = -yaw(T) only up to its 1 degree
    of pitch and half a degree of roll)."""
    from overlapnet_amd.registration import pose_from_network_yaw, pose_from_yaw_bin
    from overlapnet_amd.evaluate import yaw_bin_to_degrees
    with np.load(os.path.join(G, "gt_overlap_yaw.npz")) as z:
        poses = z["poses"]
        rows = {int(k.split("_")[1]): z[k] for k in z.files if k.startswith("mapping_")}
    n = 0
    for r_frame, table in rows.items():                   # table[c] = [r_frame as current, c as reference, overlap, bin]
        for c in range(len(poses)):
            assert int(table[c][0]) == r_frame and int(table[c][1]) == c
            argmax = int(table[c][3])                     # what the network answers with r_frame on its first leg, c on its second
            yaw_out = 180 - argmax                        # infer.py:158
            assert yaw_bin_to_degrees(argmax) == yaw_out
            T = pose_from_network_yaw(yaw_out)
            assert np.array_equal(T, R.rz(-yaw_out))      # width 360: Rz(-yaw degrees)
            rel = np.linalg.inv(poses[c]) @ poses[r_frame]               # reference r_frame into current c
            want = np.degrees(np.arctan2(rel[1, 0], rel[0, 0]))
            got = np.degrees(np.arctan2(T[1, 0], T[0, 0]))
            d = (got - want + 180.0) % 360.0 - 180.0
            assert abs(d) <= 1.05, (r_frame, c, argmax, want, got)
            n += 1
    assert n == 60
    # it is the inverse of the ground-truth pose of the same number read as a bin, at any width
    for width in (360, 180, 512):
        for y in (-100, -1, 0, 7, 180):
            assert np.allclose(pose_from_network_yaw(y, width) @ pose_from_yaw_bin(180 - y, width), np.eye(4), atol=1e-15)


def test_header_declares_and_binding_covers_icp_register():
    from overlapnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+ovn_icp_register\s*\(([^)]*)\)", src)
    assert m, "include/ovn_hip.h does not declare ovn_icp_register"
    assert len(m.group(1).split(",")) == 23
    assert "ovn_icp_register" in _lib.SIGNATURES          # (its types and arity against the header: tests/test_abi.py)
    assert re.search(r"#define\s+OVN_ABI_VERSION\s+11\b", src) and _lib.ABI_VERSION == 11
    lib = _lib.load()
    # argument errors are refused before any GPU call
    assert lib.ovn_icp_register(None, None, None, None, 0, 64, 900, 3.0, -25.0, 50.0, None, None, 0, None, 20, 2.0, 0.8, 0.2, 64,
                                None, None, None, None) == 1
    assert b"ctx is NULL" in lib.ovn_last_error()
