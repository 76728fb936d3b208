"""CPU: the statement of the TSDF ray caster (tests/_raycast_ref.py) checked on its own -- float32 against
float64 on every shared case, the brick mask against brute force -- plus the refusals of the Python surface before a GPU is touched, the
bounds rule `tools/build_mesh.py` had, the pose file and the constant-velocity prediction.  tests/test_gpu_raycast.py compares the
kernels with the same statement."""
import numpy as np
import pytest

import _raycast_ref as RC
import _render_ref as R

AMBIGUOUS_CAP = 0.02


@pytest.mark.parametrize("name,hw", RC.CASES, ids=["%s-%dx%d" % (n, h, w) for n, (h, w) in RC.CASES])
def test_f32_statement_against_f64(name, hw):
    c = RC.volume_case(name)
    f32, f64 = RC.reference(name, hw), RC.reference(name, hw, "float64")
    amb = f64["ambiguous"]
    share = float(amb.mean())
    hit32, hit64 = f32["range"] > 0, f64["range"] > 0
    print("%s %dx%d: ambiguous share %.4f of %d rays, %d hits" % (name, hw[0], hw[1], share, amb.size, int(hit64.sum())))
    assert share <= AMBIGUOUS_CAP
    clear = ~amb
    assert np.array_equal(hit32[clear], hit64[clear])
    both = hit32 & hit64 & clear
    if name != "behind":
        assert both.sum() >= 5                                                  # the case sees its surface
    bound = RC.error_bound(c["tsdf"], c["origin"], c["voxel"], c["poses"], c["max_range"], c["step"], f64["denom"])
    err = np.abs(f32["range"].astype(np.float64) - f64["range"])
    if both.any():
        print("max |t32 - t64| %.3g, smallest bound %.3g, largest bound %.3g" % (err[both].max(), bound[both].min(), bound[both].max()))
        assert np.all(err[both] <= bound[both])
        assert np.median(bound[both]) < 1e-2                                    # the bound says something: a twentieth of a voxel
    # the NaN pose is all empty, an empty pixel is -1 in every channel, a hit's vertex is (t d_s, 1)
    bad = ~np.isfinite(np.asarray(c["poses"], np.float64).astype(np.float32)[:, :3, :]).all(axis=(1, 2))
    assert np.all(f32["range"][bad] == -1)
    assert np.all(f32["vertex"][~hit32] == -1) and np.all(f32["vertex"][hit32][:, 3] == 1)
    assert np.all(f32["range"][hit32] >= np.float32(c["min_range"])) and np.all(f32["range"][hit32] < np.float32(c["max_range"]))
    # the mask route of the statement
    masked = RC.reference(name, hw, "float32", True)
    assert np.array_equal(masked["range"].view(np.uint32), f32["range"].view(np.uint32))


def test_behind_a_surface_is_empty_and_the_grid_plane_is_integer():
    c = RC.volume_case("behind")
    assert np.all(RC.reference("behind", RC.IMAGES[0])["range"] == -1)
    assert c["min_range"] > RC.volume_case("plane")["min_range"]
    g = RC.volume_case("grid_plane")
    gz = (np.float32(g["poses"][0, 2, 3]) - np.float32(g["origin"][2])) * (np.float32(1) / np.float32(g["voxel"]))
    assert gz == 3.0 and np.all(g["poses"][:, 2, :3] == 0)
    assert (RC.reference("grid_plane", RC.IMAGES[0])["range"] > 0).sum() > 100
    o = RC.volume_case("odd_step")
    k = RC.sample_count(o["min_range"], o["max_range"], o["step"])
    assert abs((o["max_range"] - o["min_range"]) / o["step"] - round((o["max_range"] - o["min_range"]) / o["step"])) > 0.05
    assert np.float32(o["min_range"]) + np.float32(k - 1) * np.float32(o["step"]) < np.float32(o["max_range"])
    assert not np.float32(o["min_range"]) + np.float32(k) * np.float32(o["step"]) < np.float32(o["max_range"])


def test_sample_count_is_the_python_surface_count():
    from overlapnet_amd import tsdf
    for mn, mx, st in ((0.5, 50.0, 0.2), (0.5, 20.0, 0.25), (0.15, 7.3, 0.185), (1.0, 1.0 + 2 ** -20, 0.5), (0.5, 0.7, 0.2), (0.5, 0.9, 0.2)):
        assert tsdf.ray_samples(mn, mx, st) == RC.sample_count(mn, mx, st) >= 1
    assert tsdf.check_march(0.5, 0.5 + 1e-3 * (2 ** 20 - 2), 1e-3) <= tsdf.MAX_RAY_SAMPLES


@pytest.mark.parametrize("shape", [(17, 9, 8), (16, 16, 16), (2, 2, 2), (9, 25, 3)])
def test_brick_mask_against_brute_force(shape):
    nx, ny, nz = shape
    g = np.random.default_rng(nx * 100 + ny)
    w = np.zeros((nz, ny, nx), np.float32)
    w.reshape(-1)[g.integers(0, w.size, 5)] = g.choice([0.5, 1.0, 2.0], 5).astype(np.float32)
    w[nz - 1, ny - 1, nx - 1] = 1.0
    for mw in (1.0, 0.5, 3.0):
        m = RC.bricks(w, mw)
        assert m.shape == (-(-nz // 8), -(-ny // 8), -(-nx // 8)) and m.dtype == np.uint8
        for bk in range(m.shape[0]):
            for bj in range(m.shape[1]):
                for bi in range(m.shape[2]):
                    blk = w[8 * bk:8 * bk + 8, 8 * bj:8 * bj + 8, 8 * bi:8 * bi + 8]
                    assert m[bk, bj, bi] == int((blk >= np.float32(mw)).any())
    assert RC.bricks(np.full((3, 3, 3), np.nan, np.float32)).sum() == 0


class _NoGpu(object):
    """An engine stand-in that fails the test when a refusal comes too late."""
    @property
    def device(self):
        raise AssertionError("the GPU was touched before the arguments were checked")

    def __getattr__(self, name):
        raise AssertionError("engine.%s was reached before the arguments were checked" % name)


def test_refusals_before_the_gpu():
    from overlapnet_amd import odometry, tsdf
    vol = tsdf.TsdfVolume.__new__(tsdf.TsdfVolume)
    vol.engine, vol.voxel, vol.n_scans = _NoGpu(), 0.2, 0
    poses = np.tile(np.eye(4), (2, 1, 1))
    nan, inf = float("nan"), float("inf")
    for kw in (dict(poses=poses[0]), dict(poses=np.zeros((2, 3, 4))), dict(poses=poses, min_range=0.0), dict(poses=poses, min_range=nan),
               dict(poses=poses, max_range=inf), dict(poses=poses, max_range=0.4), dict(poses=poses, min_range=50.0),
               dict(poses=poses, step=0.0), dict(poses=poses, step=nan), dict(poses=poses, step=1e-5), dict(poses=poses, min_weight=nan),
               dict(poses=poses, proj_h=0), dict(poses=poses, proj_w=0)):
        with pytest.raises(ValueError):
            vol.render_scans(**kw)
    with pytest.raises(ValueError):
        vol.bricks(nan)
    for kw in (dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.0), dict(lo=(0, 0, 0), hi=(1, 0, 1), voxel=0.1),
               dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, min_range=0.0), dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, max_range=0.3),
               dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, proj_h=0), dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, min_fitness=1.5),
               dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, tolerance=3), dict(lo=(0, 0, 0), hi=(2000, 2000, 200), voxel=0.05)):
        with pytest.raises(ValueError):
            odometry.TsdfOdometry(_NoGpu(), **kw)
    pts = np.zeros((10, 4), np.float32)
    for kw in (dict(points=pts[:, :3], offsets=[0, 10]), dict(points=pts, offsets=[0, 11]), dict(points=pts, offsets=[0, 6, 5]),
               dict(points=pts, offsets=[0, 5, 10], chunk=0), dict(points=pts, offsets=[0, 5, 10], proj_w=0)):
        with pytest.raises(ValueError):
            odometry.frame_to_frame(_NoGpu(), **kw)
    with pytest.raises(ValueError):
        odometry.estimate_poses(_NoGpu(), pts, [0])
    with pytest.raises(ValueError):
        odometry.estimate_poses(_NoGpu(), pts[:, :2], [0, 10])


def test_bounds_from_poses_is_the_rule_build_mesh_had():
    from overlapnet_amd import odometry
    from tools import build_mesh
    g = np.random.default_rng(3)
    poses = np.tile(np.eye(4), (7, 1, 1))
    poses[:, :3, 3] = g.normal(scale=30.0, size=(7, 3))
    for max_range, below, above in ((50.0, 5.0, 15.0), (20.0, 1.0, 2.5)):
        o = poses[:, :3, 3]
        lo, hi = o.min(axis=0), o.max(axis=0)                     # the rule as tools/build_mesh.py stated it
        want = (np.array([lo[0] - max_range, lo[1] - max_range, lo[2] - below]),
                np.array([hi[0] + max_range, hi[1] + max_range, hi[2] + above]))
        for got in (odometry.bounds_from_poses(poses, max_range, below, above), build_mesh.default_bounds(poses, max_range, below, above)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    d = odometry.bounds_from_poses(poses, 50.0)
    assert d[0][2] == poses[:, 2, 3].min() - 5.0 and d[1][2] == poses[:, 2, 3].max() + 15.0


def test_pose_file_round_trip(tmp_path):
    from overlapnet_amd import odometry
    from tools.build_training_set import read_poses
    g = np.random.default_rng(11)
    poses = np.stack([R.pose_at(*g.uniform(-50, 50, 2), z=g.uniform(0, 2), yaw=g.uniform(-3, 3)) for _ in range(5)])
    poses[0] = np.eye(4)
    path = tmp_path / "poses.txt"
    odometry.write_poses(str(path), poses)
    lines = path.read_text().strip().splitlines()
    assert len(lines) == 5 and all(len(ln.split()) == 12 for ln in lines)
    assert lines[0].split() == ["1.0", "0.0", "0.0", "0.0", "0.0", "1.0", "0.0", "0.0", "0.0", "0.0", "1.0", "0.0"]
    back = read_poses(str(path))
    assert back.shape == (5, 4, 4) and np.array_equal(back, poses)
    with pytest.raises(ValueError):
        odometry.write_poses(str(path), poses[0])


def test_constant_velocity_prediction_on_a_screw_motion():
    """T_k = S^k for a screw S (a turn about a tilted axis plus a slide along it): the prediction from T_1, T_2 is T_3."""
    import _icp_ref as I
    from overlapnet_amd import odometry
    S = I.se3_exp(np.array([0.3, -0.1, 0.2, 0.02, -0.05, 0.11]))
    start = R.pose_at(3.0, -2.0, yaw=0.7)
    T = [start]
    for _ in range(3):
        T.append(T[-1] @ S)
    pred = odometry.predict(T[1], T[2])
    assert np.allclose(pred, T[3], rtol=0, atol=1e-12)
    assert np.allclose(pred[:3, :3] @ pred[:3, :3].T, np.eye(3), atol=1e-12)
    assert np.array_equal(odometry.predict(T[1], T[1]), T[1] @ (np.linalg.inv(T[1]) @ T[1]))
    assert np.allclose(odometry.predict(np.eye(4), np.eye(4)), np.eye(4), atol=0)
