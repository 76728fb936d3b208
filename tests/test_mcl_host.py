"""CPU: the host side of the Monte Carlo localization -- the Philox restatement against the published known answers, the integer
resampler's guarantees, map building, and the sign of the expected yaw.  (The kernels: tests/test_gpu_mcl.py.)"""
import math

import numpy as np
import pytest

import _mcl_ref as R
from overlapnet_amd import ground_truth as GT
from overlapnet_amd import localization as L


def test_philox_known_answers():
    for counter, key, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(counter, key)
        assert [int(v) for v in got] == list(want), (counter, key, [hex(int(v)) for v in got])
    # vectorised over the first counter word: row i is the scalar call with counter (i, ...)
    many = R.motion_words(5, seed=0x1234567890ABCDEF, step=(7 << 32) | 3)
    for i in range(5):
        one = R.philox4x32_10((i, 3, 7, 0), (0x90ABCDEF, 0x12345678))
        assert np.array_equal(many[i], one)


def test_uniform_is_inside_the_unit_interval():
    w = np.array([0, 255, 256, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)
    for arith in (np.float32, np.float64):
        u = R.uniform(w, arith)
        assert u.dtype == arith and np.all(u > 0) and np.all(u <= 1)      # ln u is finite
    assert R.uniform(w, np.float64)[0] == 2.0 ** -25 and R.uniform(w, np.float32)[0] == np.float32(2.0 ** -25)


def _weights(P, kind, g):
    if kind == "one":
        w = np.zeros(P, np.float32)
        w[g.integers(0, P)] = 0.75
    elif kind == "equal":
        w = np.full(P, 0.5, np.float32)
    elif kind == "third_zero":
        w = g.uniform(0.0, 1.0, P).astype(np.float32)
        w[::3] = 0.0
        w[g.integers(0, P)] = 0.9
    else:
        w = g.uniform(0.0, 1.0, P).astype(np.float32)
        w[g.integers(0, P)] = 0.6
    return w


@pytest.mark.parametrize("P,n_out", [(1, 1), (2, 3), (65, 64), (65536, 100)])
def test_resampler_reference_properties(P, n_out):
    g = np.random.default_rng(P * 7 + n_out)
    for kind in ("one", "equal", "third_zero", "random"):
        w = _weights(P, kind, g)
        for step in (0, 5):
            anc, rec = R.resample(w, n_out, R.resample_offset_words(seed=11, step=step))
            assert list(rec) == [0, n_out, 0, 1]
            R.check_resample_properties(w, n_out, anc)
    # negative, NaN and infinite weights count as zero; nothing positive: status 1
    bad = np.array([np.nan, -1.0, np.inf, 0.0][:max(1, min(P, 4))], np.float32)
    anc, rec = R.resample(bad, n_out, R.resample_offset_words(1, 1))
    assert anc is None and list(rec) == [1, 0, 0, 1]


def test_map_cells_take_the_nearest_frame_within_reach():
    xy = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 6.0]])
    res, reach = 2.0, 2.0
    ox, oy, nx, ny = L.grid_for(xy, res, reach)
    table = L.build_cell_frame(xy, ox, oy, res, nx, ny, reach).reshape(ny, nx)
    cx = ox + (np.arange(nx) + 0.5) * res
    cy = oy + (np.arange(ny) + 0.5) * res
    for iy in range(ny):
        for ix in range(nx):
            d = np.hypot(xy[:, 0] - cx[ix], xy[:, 1] - cy[iy])
            want = int(np.argmin(d)) if d.min() <= reach else -1
            assert table[iy, ix] == want, (ix, iy, d)
    assert (table == -1).any() and set(np.unique(table)) == {-1, 0, 1, 2}      # cells beyond reach of every frame are empty
    # every frame's own cell exists in the grid and names a frame within reach of its centre
    cells = L.cell_of(xy[:, 0], xy[:, 1], ox, oy, res, nx, ny)
    assert np.all(cells >= 0) and np.all(table.reshape(-1)[cells] >= 0)


def test_a_frame_on_a_cell_border_lands_in_exactly_one_cell():
    res = 0.5
    xy = np.array([[1.0, 2.5], [3.0, 2.5]])              # both exactly on cell borders in x and y
    ox, oy, nx, ny = L.grid_for(xy, res, res)
    for x, y in xy:
        c = int(L.cell_of([x], [y], ox, oy, res, nx, ny)[0])
        ix, iy = c % nx, c // nx
        # the cell whose lower border the position is on, and no other: [ox + ix res, ox + (ix + 1) res)
        assert ox + ix * res == x and oy + iy * res == y
        below = np.nextafter(np.float32(x), np.float32(-np.inf))
        assert int(L.cell_of([below], [y], ox, oy, res, nx, ny)[0]) == c - 1
    # outside the grid on every side, and non-finite coordinates: no cell
    far = L.cell_of([ox - 1e-3, ox + nx * res, 1.0, 1.0, np.nan, np.inf], [2.5, 2.5, oy - 1e-3, oy + ny * res, 2.5, 2.5],
                    ox, oy, res, nx, ny)
    assert np.all(far == -1)
    # the library's lookup restated in the reference agrees with the product's
    table = L.build_cell_frame(xy, ox, oy, res, nx, ny, res)
    g = np.random.default_rng(0)
    px, py = g.uniform(ox - 1, ox + nx * res + 1, 500), g.uniform(oy - 1, oy + ny * res + 1, 500)
    cells = L.cell_of(px, py, ox, oy, res, nx, ny)
    want = np.where(cells >= 0, table[np.maximum(cells, 0)], -1)
    assert np.array_equal(R.lookup(px, py, table, ox, oy, res, nx, ny, 2), want)


def _pose(x, y, yaw):
    T = np.eye(4)
    T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    T[:2, 3] = x, y
    return T


def test_expected_yaw_of_a_particle_is_theta_minus_psi():
    """`Infer` puts the map frame (the reference) on head-left and the query (the current frame) on head-right and returns
    180 - argmax; argmax is the ground-truth bin of the SWAPPED pair (registration.pose_from_network_yaw).  So the yaw the
    network reports for a particle at heading theta against a frame at heading psi is 180 - yaw_bin(reference, current), which
    must be wrap(theta - psi) in degrees to within one bin."""
    for theta, psi in [(0.3, 0.1), (-2.0, 2.5), (3.0, -3.0), (1.0, 1.0), (-0.5, 0.7), (2.9, 0.2), (0.0, -1.6)]:
        reference, current = _pose(5.0, -2.0, psi), _pose(5.5, -1.0, theta)
        network = 180 - GT.yaw_bin(reference, current)
        want = math.degrees(float(R.angle_diff(theta, psi)))
        d = (network - want + 180.0) % 360.0 - 180.0
        assert abs(d) <= 1.0, (theta, psi, network, want)
        # and the other sign is wrong wherever the angle is not small
        if abs(want) > 2.0 and abs(abs(want) - 180.0) > 2.0:
            assert abs((network + want + 180.0) % 360.0 - 180.0) > 1.0


def test_observation_model_prefers_the_matching_heading():
    P = 8
    parts = np.zeros((P, 4), np.float32)
    parts[:, 2] = np.radians([0, 10, 20, 30, 90, 180, -30, -10])
    parts[:, 3] = 1.0
    psi = np.array([0.0], np.float32)
    prod, on = R.products(parts, np.zeros(P, np.int32), np.array([0], np.int32), psi, np.array([0.5], np.float32),
                          np.array([20], np.int32), sigma_yaw=5.0, eps_yaw=0.01, overlap_min=0.05)
    assert on.all() and int(np.argmax(prod)) == 2
    w, status = R.rescale(prod)
    assert status == 0 and 0.5 <= w.max() < 1.0 and np.array_equal(np.argsort(prod), np.argsort(w))
    assert R.rescale(np.zeros(4))[1] == 1


def test_float32_figures_behind_the_gpu_tolerances():
    """tests/test_gpu_mcl.py allows the GPU ten times the distance between this reference in float32 and in fp64 on its inputs; the
    figures written there (R.F32_PREDICT, R.F32_WEIGHT) are those distances rounded up -- recomputed here."""
    worst = [0.0, 0.0]
    for P in R.PREDICT_SIZES:
        parts, words = R.predict_case(P), R.motion_words(P, R.PREDICT_SEED, R.PREDICT_STEP)
        for sigma in (R.PREDICT_SIGMA, (0.0, 0.0, 0.0)):
            lo = R.predict(parts, words, R.PREDICT_ODOM, sigma, np.float32)
            assert lo.dtype == np.float32
            e = R.predict_error(lo, R.predict(parts, words, R.PREDICT_ODOM, sigma, np.float64))
            worst = [max(a, b) for a, b in zip(worst, e)]
    assert 0.25 * R.F32_PREDICT[0] < worst[0] <= R.F32_PREDICT[0] and 0.25 * R.F32_PREDICT[1] < worst[1] <= R.F32_PREDICT[1], worst
    dw = 0.0
    for P in R.UPDATE_SIZES:
        case = R.update_case(P)
        lo, on, status = R.update_weights(case, np.float32)
        hi, _, _ = R.update_weights(case, np.float64)
        assert lo.dtype == np.float32 and status == 0 and 0.5 <= hi.max() < 1.0 and hi.min() > 2.0 ** -100
        dw = max(dw, float(np.abs(lo.astype(np.float64) - hi).max()))
        th = case["particles"][:, 2].astype(np.float64)
        assert np.hypot((hi * np.sin(th)).sum(), (hi * np.cos(th)).sum()) / hi.sum() >= 0.1      # the heading test's precondition
    assert 0.25 * R.F32_WEIGHT < dw <= R.F32_WEIGHT, dw


def test_localize_tool_reads_rows_and_refuses_a_sharded_infer(tmp_path):
    from tools import localize
    from overlapnet_amd._lib import OvnError
    f = tmp_path / "odom.txt"
    f.write_text("# frame dx dy dtheta\n000001 0.5 0.0 0.01\n\n000002 0.6 -0.1 -0.02   # a comment\n")
    names, rows = localize.read_rows(str(f))
    assert names == ["000001", "000002"] and np.array_equal(rows, [[0.5, 0.0, 0.01], [0.6, -0.1, -0.02]])
    f.write_text("000001 0.5 0.0\n")
    with pytest.raises(ValueError):
        localize.read_rows(str(f))
    with pytest.raises(SystemExit):
        localize.main(["--config", "x.json", "--map", "m.npz"])        # neither --build nor --odom

    class Sharded(object):
        _world = 4
    with pytest.raises(OvnError, match="sharded"):
        L.OverlapMap(Sharded(), ["0"], np.zeros((1, 3)), 1.0)
    assert np.allclose(L.poses_xyyaw(np.stack([_pose(1.0, 2.0, 0.5)])), [[1.0, 2.0, 0.5]], rtol=0, atol=1e-15)
