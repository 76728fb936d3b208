"""GPU (MI355X), end to end: a closed drive through the test scene, loop closures by the GPU ICP, the pose graph optimized on the GPU.

The drive: 14 scans at 32 x 360 on a circle of radius 2.5 m in the scene of tests/_render_ref.py (every position at least 0.7 m from
every box and wall), heading along the tangent; scan 13 is one step short of scan 0, so the drive returns to its start.
  odometry edges  the true steps with a constant yaw bias of 0.2 degrees per step composed in: dead reckoning does not close
  loop edges      `register_scans` between the last two and the first two scans -- (13, 0), (13, 1), (12, 0), (12, 1) -- each started from
                  the true relative pose turned by 3 degrees about z
  information     odometry and loops alike from sigmas 0.05 m / 0.01 rad
The reference optimizer (tests/_pose_graph_ref.py, dense solves) runs on the CPU on the very edges the GPU produced.  The GPU result
must lie within ten times OPT_FIGURE of it (tests/test_gpu_pose_graph.py: the reference with its own PCG against the reference with a
dense solve, 1.4e-9), and its largest position error against the true poses must be below dead reckoning's by the factor the reference
achieves, less 10 %.  tests/golden/pose_graph_loop.json records both errors as measured on an MI355X: dead reckoning 0.1205 m, the
reference 0.0043 m (a factor 27.8; the GPU ends 1.8e-15 from the reference; the loop registrations themselves are within 2.5 mm)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _pose_graph_ref as PR
from tests import _render_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

HW = (32, 360)
N_SCANS, RADIUS, CLEARANCE = 14, 2.5, 0.7
BIAS_DEG, START_DEG = 0.2, 3.0
SIGMA_T, SIGMA_R = 0.05, 0.01
LOOPS = [(13, 0), (13, 1), (12, 0), (12, 1)]
ICP = dict(iterations=20, max_dist=2.0, cos_min=0.8, huber=0.2, min_inliers=64)
OPT_FIGURE = 1.4e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_loop.json")


def closed_drive(seed=0):
    """The true poses (14,4,4): the first circle of a seeded search that keeps its clearance."""
    g = np.random.default_rng([seed, 11])
    blo, bhi = R.scene_boxes(0)
    ang = 2.0 * np.pi * np.arange(N_SCANS) / N_SCANS
    while True:
        cx, cy = g.uniform(RADIUS + 1.0, R.ROOM[0] - RADIUS - 1.0), g.uniform(RADIUS + 1.0, R.ROOM[1] - RADIUS - 1.0)
        xs, ys = cx + RADIUS * np.cos(ang), cy + RADIUS * np.sin(ang)
        if not np.any((xs[:, None] > blo[None, :, 0] - CLEARANCE) & (xs[:, None] < bhi[None, :, 0] + CLEARANCE) &
                      (ys[:, None] > blo[None, :, 1] - CLEARANCE) & (ys[:, None] < bhi[None, :, 1] + CLEARANCE)):
            break
    return np.stack([R.pose_at(x, y, R.SENSOR_Z, a + 0.5 * np.pi) for x, y, a in zip(xs, ys, ang)])


def _rot_z(deg):
    T = np.eye(4)
    T[:3, :3] = R._rot_z(np.radians(deg))
    return T


def _max_position_error(poses, true):
    return float(np.linalg.norm(poses[:, :3, 3] - true[:, :3, 3], axis=1).max())


def test_loop_closures_pull_a_biased_drive_back(capsys):
    from overlapnet_amd.engine import OvnEngine
    from overlapnet_amd.mesh import TriangleMesh
    from overlapnet_amd.pose_graph import PoseGraph, information_from_sigmas
    from overlapnet_amd.registration import register_scans
    eng = OvnEngine(64, 900, 4, device=0)
    try:
        true = closed_drive()
        r = eng.render_scans(TriangleMesh(*R.scene(0)), true, HW[0], HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
        rng, vtx = r["range"].cpu().numpy(), r["vertex"].cpu().numpy()
        clouds = [np.ascontiguousarray(vtx[s][rng[s] > 0], np.float32) for s in range(N_SCANS)]
        steps = [PR.mul_se3(PR.rel_se3(true[k], true[k + 1]), _rot_z(BIAS_DEG)) for k in range(N_SCANS - 1)]
        dead = [true[0]]
        for Z in steps:
            dead.append(PR.mul_se3(dead[-1], Z))
        dead = np.stack(dead)
        # edge (cur, ref, Z): Z takes the reference scan's points into the current scan's frame = T_cur^-1 T_ref; source = ref, target = cur
        init = np.stack([PR.mul_se3(PR.rel_se3(true[c], true[f]), _rot_z(START_DEG)) for c, f in LOOPS])
        regs = register_scans(eng, clouds, [(f, c) for c, f in LOOPS], init, proj_H=HW[0], proj_W=HW[1], fov_up=R.FOV_UP,
                              fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE, **ICP)
        assert all(g.status == 0 for g in regs)
        om = information_from_sigmas(SIGMA_T, SIGMA_R)
        pg = PoseGraph(eng, dead)
        pg.add_odometry(np.stack(steps), om)
        for (c, f), g in zip(LOOPS, regs):
            pg.add_edge(c, f, g.pose, om)
        res = pg.optimize()
        edges, Z = pg.edges, np.stack(steps + [g.pose for g in regs])
        fixed = np.zeros(N_SCANS, bool)
        fixed[0] = True
        want = PR.optimize(dead, fixed, edges, Z, np.stack([om] * len(edges)), max_iterations=30, solver="dense")
        e_dead, e_ref, e_gpu = (_max_position_error(p, true) for p in (dead, want["poses"], res.poses))
        icp = max(float(np.linalg.norm(g.pose[:3, 3] - PR.rel_se3(true[c], true[f])[:3, 3])) for (c, f), g in zip(LOOPS, regs))
        with capsys.disabled():
            print("\nSLAM: largest position error: dead reckoning %.6f m, reference %.6f m, GPU %.6f m; GPU against the reference %.3g; "
                  "largest ICP translation error %.4f m; %d outer / %d PCG iterations (%s), cost %.6g -> %.6g"
                  % (e_dead, e_ref, e_gpu, np.abs(res.poses - want["poses"]).max(), icp, res.outer_iterations, res.cg_iterations,
                     pg.choose_preconditioner("auto"), res.cost_initial, res.cost_final))
        assert res.converged and want["converged"]
        assert e_ref < e_dead, "the reference does not improve on dead reckoning: the drive is wrong, not the bound"
        assert np.abs(res.poses - want["poses"]).max() <= 10 * OPT_FIGURE
        factor = e_dead / e_ref
        assert e_gpu <= e_dead / (0.9 * factor)
        with open(GOLDEN) as f:
            gold = json.load(f)
        assert abs(e_dead - gold["dead_reckoning_max_position_error_m"]) <= 1e-9            # arithmetic on the true poses alone
        assert abs(e_ref - gold["reference_max_position_error_m"]) <= 1e-6                  # the GPU ICP gives the same bits every run
    finally:
        torch.cuda.synchronize()
        eng.close()
