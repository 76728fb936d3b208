"""CPU: the NumPy restatement of the `TsdfOdometry` loop (tests/_odometry_ref.py) on the seeded drive, against the true poses and
against the record tests/test_gpu_odometry.py takes its bound from (tests/golden/odometry_ref.json)."""
import json
import os

import numpy as np

import _odometry_ref as OD
import _render_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "odometry_ref.json")


def test_drive_keeps_clear_of_boxes_and_walls():
    world, rel = OD.drive()
    rot = R._rot_z(R.SCENE_ROT)
    xy = (world[:, :3, 3] @ rot)[:, :2]                                  # back into the room's frame
    blo, bhi = R.scene_boxes(0)
    assert xy.min() >= OD.CLEARANCE - 1e-9 and np.all(xy[:, 0] <= R.ROOM[0] - OD.CLEARANCE) and np.all(xy[:, 1] <= R.ROOM[1] - OD.CLEARANCE)
    d = np.maximum(np.maximum(blo[None, :, :2] - xy[:, None, :], xy[:, None, :] - bhi[None, :, :2]), 0.0)
    assert np.sqrt((d ** 2).sum(-1)).min() >= OD.CLEARANCE - 1e-9
    assert np.allclose(np.linalg.norm(np.diff(xy, axis=0), axis=1), OD.STEP_M) and np.array_equal(rel[0], np.eye(4))


def test_restatement_tracks_the_drive_and_is_the_record():
    world, rel = OD.drive()
    rng, vtx = OD.scans()
    lo, hi = OD.volume_box(world[0])
    poses, sources = OD.track(rng, vtx, lo, hi)
    dt, dr = OD.distances(poses, rel)
    print("restatement: translation %s m, rotation %s deg" % (np.round(dt, 5).tolist(), np.round(dr, 5).tolist()))
    assert sources == ["first"] + ["model"] * (OD.N_FRAMES - 1)
    assert dt.max() < 0.05 and dr.max() < 0.5                            # it tracks: a tenth of a step, a third of a turn
    with open(GOLDEN) as f:
        gold = json.load(f)
    # the record the GPU test's bound is taken from: the same figures, up to what another libm moves a registration by
    assert gold["sources"] == sources
    assert abs(gold["max_translation_m"] - dt.max()) <= 0.1 * gold["max_translation_m"]
    assert abs(gold["max_rotation_deg"] - dr.max()) <= 0.1 * gold["max_rotation_deg"]
