"""GPU: the LiDAR odometry (overlapnet_amd/odometry.py) on a seeded drive through the test scene: the
frame-to-model tracker against its NumPy restatement (tests/_odometry_ref.py), `frame_to_frame` against per-pair registrations, run-to-
run bits, an empty scan in the middle, and tools/odometry.py end to end.

The bound of the tracker: the restatement's own largest distance from the true poses is recorded in tests/golden/odometry_ref.json
(tests/test_odometry_host.py recomputes it on the CPU): 0.0147 m and 0.124 degrees.  Every frame of the GPU trajectory must lie within
TWICE that of the truth, in translation and in rotation -- twice, because an association that flips between the float32 kernel and the
float64 statement moves a registration by more than rounding."""
import json
import os

import numpy as np
import pytest
import torch

import _icp_ref as I
import _odometry_ref as OD
import _render_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

SENSOR = dict(proj_h=OD.HW[0], proj_w=OD.HW[1], fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "odometry_ref.json")


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def drive(eng):
    """The drive as raw clouds, rendered on the GPU (the renderer gives the bits of its statement: tests/test_gpu_render.py)."""
    from overlapnet_amd.mesh import TriangleMesh
    world, rel = OD.drive()
    r = eng.render_scans(TriangleMesh(*R.scene(0)), world, OD.HW[0], OD.HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
    rng, vtx = r["range"].cpu().numpy(), r["vertex"].cpu().numpy()
    clouds = [np.ascontiguousarray(vtx[s][rng[s] > 0], np.float32) for s in range(OD.N_FRAMES)]
    offsets = np.zeros(OD.N_FRAMES + 1, np.int64)
    offsets[1:] = np.cumsum([c.shape[0] for c in clouds])
    lo, hi = OD.volume_box(world[0])
    return dict(world=world, rel=rel, clouds=clouds, points=np.concatenate(clouds), offsets=offsets, lo=lo, hi=hi)


def _tracker(eng, drive):
    from overlapnet_amd import odometry
    return odometry.TsdfOdometry(eng, drive["lo"], drive["hi"], OD.VOXEL, trunc=OD.TRUNC, min_range=OD.MIN_RANGE, **SENSOR, **OD.ICP)


@pytest.fixture(scope="module")
def tracked(eng, drive):
    odo = _tracker(eng, drive)
    results = [odo.track(c) for c in drive["clouds"]]
    return odo, results


def test_drive_is_as_stated(drive):
    rel = drive["rel"]
    steps = [I.pose_error(rel[i + 1], rel[i]) for i in range(OD.N_FRAMES - 1)]
    assert np.allclose([s[0] for s in steps], OD.STEP_M, atol=1e-9) and np.allclose([s[1] for s in steps], OD.YAW_DEG, atol=1e-6)
    assert np.allclose(rel[0], np.eye(4), atol=1e-12) and all(c.shape[0] > 0.5 * OD.HW[0] * OD.HW[1] for c in drive["clouds"])


def test_tracker_stays_within_twice_the_restatement_of_the_truth(tracked, drive):
    odo, results = tracked
    with open(GOLDEN) as f:
        gold = json.load(f)
    poses = np.stack([r.pose for r in results])
    dt, dr = OD.distances(poses, drive["rel"])
    print("GPU trajectory: translation %s m, rotation %s deg; restatement max %.5f m, %.5f deg; sources %s"
          % (np.round(dt, 5).tolist(), np.round(dr, 5).tolist(), gold["max_translation_m"], gold["max_rotation_deg"],
             [r.source for r in results]))
    assert results[0].source == "first" and np.array_equal(results[0].pose, np.eye(4))
    assert [r.source for r in results[1:]] == ["model"] * (OD.N_FRAMES - 1) and all(r.status == 0 for r in results)
    assert np.all(dt <= 2.0 * gold["max_translation_m"])
    assert np.all(dr <= 2.0 * gold["max_rotation_deg"])
    assert odo.volume.n_scans == OD.N_FRAMES and all(0.0 < r.fitness <= 1.0 for r in results[1:])


def test_two_runs_give_the_same_bits(eng, drive, tracked):
    odo = _tracker(eng, drive)
    again = [odo.track(c) for c in drive["clouds"]]
    for a, b in zip(again, tracked[1]):
        assert np.array_equal(a.pose.view(np.uint64), b.pose.view(np.uint64)) and a[1:] == b[1:]
    assert torch.equal(odo.volume.tsdf.view(torch.int32), tracked[0].volume.tsdf.view(torch.int32))


def test_frame_to_frame_equals_per_pair_registrations(eng, drive):
    from overlapnet_amd import odometry
    from overlapnet_amd.registration import register_scans
    n = OD.N_FRAMES
    poses, regs = odometry.frame_to_frame(eng, drive["points"], drive["offsets"], **SENSOR, **OD.ICP)
    chunked, regs5 = odometry.frame_to_frame(eng, drive["points"], drive["offsets"], chunk=5, **SENSOR, **OD.ICP)
    sensor = dict(proj_H=OD.HW[0], proj_W=OD.HW[1], fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)
    assert len(regs) == len(regs5) == n - 1 and poses.shape == (n, 4, 4)
    for i in range(n - 1):
        one = register_scans(eng, drive["clouds"][i:i + 2], [(1, 0)], np.eye(4)[None], **sensor, **OD.ICP)[0]
        for r in (regs[i], regs5[i]):
            assert np.array_equal(r.pose.view(np.uint64), one.pose.view(np.uint64)), i
            assert r[1:] == one[1:], i
    assert np.array_equal(poses.view(np.uint64), chunked.view(np.uint64))
    chain = [np.eye(4)]
    for r in regs:
        assert r.status == 0
        chain.append(chain[-1] @ r.pose)
    assert np.array_equal(poses, np.stack(chain))
    dt, dr = OD.distances(poses, drive["rel"])
    print("frame to frame: translation %s m, rotation %s deg" % (np.round(dt, 4).tolist(), np.round(dr, 4).tolist()))
    assert dt.max() < 0.25 and dr.max() < 1.0            # a trajectory, not a bound: 12 chained steps of 0.5 m each


def test_an_empty_scan_in_the_middle(eng, drive):
    from overlapnet_amd import odometry
    odo = _tracker(eng, drive)
    for c in drive["clouds"][:5]:
        odo.track(c)
    before_t, before_w, fused = odo.volume.tsdf.clone(), odo.volume.weight.clone(), odo.volume.n_scans
    want = odometry.predict(odo.poses[-2], odo.poses[-1])
    res = odo.track(np.zeros((0, 4), np.float32))
    assert res.source == "prediction" and res.status != 0 and res.inliers == 0
    assert np.array_equal(res.pose, want)
    assert torch.equal(odo.volume.tsdf.view(torch.int32), before_t.view(torch.int32))
    assert torch.equal(odo.volume.weight.view(torch.int32), before_w.view(torch.int32)) and odo.volume.n_scans == fused
    nxt = odo.track(drive["clouds"][6])
    assert nxt.source == "model" and nxt.status == 0
    dt, dr = I.pose_error(nxt.pose, drive["rel"][6])
    print("after the empty scan: frame 6 is %.4f m, %.4f deg from the truth" % (dt, dr))
    assert dt < 0.05 and dr < 0.5
    with pytest.raises(ValueError):
        odo.track(drive["clouds"][7], first_pose=np.eye(4))


def test_odometry_tool_writes_poses_build_mesh_accepts(drive, tracked, tmp_path, capsys):
    from overlapnet_amd.mesh import TriangleMesh
    from tools import build_mesh
    from tools import odometry as tool
    from tools.build_training_set import read_poses
    scans = tmp_path / "scans"
    scans.mkdir()
    for s, c in enumerate(drive["clouds"]):
        c.tofile(str(scans / ("%06d.bin" % s)))
    cfg = tmp_path / "network.json"
    cfg.write_text(json.dumps({"model": {"inputShape": [OD.HW[0], OD.HW[1], 4]}}))
    out, ply = tmp_path / "poses.txt", tmp_path / "site.ply"
    common = ["--config", str(cfg), "--scans", str(scans), "--max-range", str(R.MAX_RANGE)]
    tool.main(common + ["--out", str(out), "--voxel", "0.2", "--below", "3", "--above", "4", "--mesh", str(ply)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    poses = read_poses(str(out))
    assert poses.shape == (OD.N_FRAMES, 4, 4) and np.array_equal(poses[0], np.eye(4))
    assert line["mode"] == "frame_to_model" and line["sources"]["model"] == OD.N_FRAMES - 1 and line["scans"] == OD.N_FRAMES
    dt, dr = OD.distances(poses, drive["rel"])
    print("tools/odometry.py: translation max %.4f m, rotation max %.4f deg, volume %s" % (dt.max(), dr.max(), line["volume"]))
    assert dt.max() < 0.05 and dr.max() < 0.5
    assert TriangleMesh.from_ply(str(ply)).n_triangles == line["triangles"] > 1000
    f2f = tmp_path / "f2f.txt"
    tool.main(common + ["--out", str(f2f), "--frame-to-frame-only"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["failed_pairs"] == 0
    assert read_poses(str(f2f)).shape == (OD.N_FRAMES, 4, 4)
    mesh = tmp_path / "mesh.ply"
    build_mesh.main(common + ["--poses", str(out), "--voxel", "0.2", "--below", "3", "--above", "4", "--out", str(mesh)])
    built = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert built["scans"] == OD.N_FRAMES and built["triangles"] == TriangleMesh.from_ply(str(mesh)).n_triangles > 1000
