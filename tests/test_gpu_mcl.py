"""GPU (MI355X): the Monte Carlo localization kernels (csrc/mcl.hip: `ovn_mcl_predict`, `ovn_mcl_update`, `ovn_mcl_resample`) against
the NumPy statement of the same stages (tests/_mcl_ref.py), and `MonteCarloLocalizer.step` against the stages chained by hand.

Tolerances of the fp32 stages, by the rule of tests/test_gpu_icp.py: the kernels' per-particle arithmetic is fp32, the reference's
fp64; how far that moves a result is measured on the reference itself, in NumPy float32 against fp64 on the inputs used here
(tests/test_mcl_host.py recomputes the figures), and the GPU is allowed ten times that, for another logf / sinf / cosf / expf.
  predict: the float32 reference ends at most 2.04e-6 m and 1.43e-7 rad from the fp64 one -> F32_PREDICT = (2.1e-6, 1.5e-7), the GPU
           is allowed (2.1e-5 m, 1.5e-6 rad), with and without noise;
  update:  scaled weights (maximum in [0.5, 1)) at most 1.14e-6 apart -> F32_WEIGHT = 1.2e-6, the GPU is allowed 1.2e-5.
Everything discrete (frames, lists, records, ancestors, resampled particles) is compared exactly; the fp64 sums are compared with the
GPU's own weight bits as input, within P 2^-52 of the sum of the absolute terms -- the bound between any two summation orders."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mcl_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

PREDICT_TOL = (10 * R.F32_PREDICT[0], 10 * R.F32_PREDICT[1])      # R.F32_PREDICT = (2.1e-6 m, 1.5e-7 rad)
WEIGHT_TOL = 10 * R.F32_WEIGHT                                    # R.F32_WEIGHT = 1.2e-6
U52 = 2.0 ** -52


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


def _dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


ONE_CELL = dict(cell_frame=np.array([0], np.int32), origin=(-1000.0, -1000.0), resolution=2000.0, nx=1, ny=1, n_frames=1)


def _predict(eng, parts, grid, odom=R.PREDICT_ODOM, sigma=R.PREDICT_SIGMA, seed=R.PREDICT_SEED, step=R.PREDICT_STEP):
    """-> (moved particles, particle_frame, frame_slot, frame_list, record) as NumPy arrays."""
    d = _dev(eng, parts)
    pf, slot, lst, rec = eng.mcl_predict(d, odom, sigma, seed, step, _dev(eng, grid["cell_frame"]), grid["origin"], grid["resolution"],
                                         grid["nx"], grid["ny"], grid["n_frames"])
    return tuple(t.cpu().numpy() for t in (d, pf, slot, lst, rec))


# ---- predict -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", R.PREDICT_SIZES)
def test_predict_matches_the_fp64_reference(eng, P):
    parts = R.predict_case(P)
    words = R.motion_words(P, R.PREDICT_SEED, R.PREDICT_STEP)
    for sigma in (R.PREDICT_SIGMA, (0.0, 0.0, 0.0)):
        got = _predict(eng, parts, ONE_CELL, sigma=sigma)[0]
        want = R.predict(parts, words, R.PREDICT_ODOM, sigma, np.float64)
        dpos, dth = R.predict_error(got, want)
        print("P %d sigma %s: GPU vs fp64 %.3g m %.3g rad (allowed %.3g / %.3g)" % (P, sigma, dpos, dth, *PREDICT_TOL))
        assert np.all(np.isfinite(got))
        assert dpos <= PREDICT_TOL[0] and dth <= PREDICT_TOL[1]
        assert np.all(got[:, 2] > -np.pi - 1e-6) and np.all(got[:, 2] <= np.float32(np.pi))
        assert np.array_equal(got[:, 3], parts[:, 3])                      # w untouched
        if sigma[0] == 0.0:                                                # the noiseless motion, stated directly
            th = parts[:, 2].astype(np.float64)
            dx, dy, dt = (float(np.float32(v)) for v in R.PREDICT_ODOM)
            x = parts[:, 0] + np.cos(th) * dx - np.sin(th) * dy
            y = parts[:, 1] + np.sin(th) * dx + np.cos(th) * dy
            assert np.abs(got[:, 0] - x).max() <= PREDICT_TOL[0] and np.abs(got[:, 1] - y).max() <= PREDICT_TOL[0]
            assert np.abs(R.angle_diff(got[:, 2], th + dt)).max() <= PREDICT_TOL[1]
    # the noise is there, particle by particle, and differs between steps
    noisy = _predict(eng, parts, ONE_CELL)[0]
    again = _predict(eng, parts, ONE_CELL)
    assert np.array_equal(noisy.view(np.int32), again[0].view(np.int32))   # same call, same bits
    other = _predict(eng, parts, ONE_CELL, step=R.PREDICT_STEP + 1)[0]
    assert not np.array_equal(noisy[:, :3], other[:, :3])


# ---- lookup and distinct list ------------------------------------------------------------------------------------------------------
def _holes_grid():
    g = np.random.default_rng(5)
    table = g.integers(0, 9, 35).astype(np.int32)
    table[[0, 6, 12, 17, 23, 34]] = -1
    return dict(cell_frame=table, origin=(-3.5, -2.5), resolution=1.0, nx=7, ny=5, n_frames=9)


def _wide_grid():
    table = np.arange(64 * 33, dtype=np.int32)
    table[table >= 2049] = -1
    return dict(cell_frame=table, origin=(-16.0, -8.25), resolution=0.5, nx=64, ny=33, n_frames=2049)


def _spread_particles(P, grid, seed, margin):
    g = np.random.default_rng(seed)
    x0, y0 = grid["origin"]
    x1, y1 = x0 + grid["nx"] * grid["resolution"], y0 + grid["ny"] * grid["resolution"]
    p = np.empty((P, 4), np.float32)
    p[:, 0], p[:, 1] = g.uniform(x0 - margin, x1 + margin, P), g.uniform(y0 - margin, y1 + margin, P)
    p[:, 2] = -g.uniform(-np.pi, np.pi, P)
    p[:, 3] = 1.0
    return p


def _check_lookup(eng, parts, grid):
    got, pf, slot, lst, rec = _predict(eng, parts, grid, odom=(0.3, 0.1, 0.2), sigma=(0.2, 0.2, 0.1))
    want_pf = R.lookup(got[:, 0], got[:, 1], grid["cell_frame"], grid["origin"][0], grid["origin"][1], grid["resolution"], grid["nx"],
                       grid["ny"], grid["n_frames"])
    want_lst, want_slot, want_rec = R.distinct(want_pf, grid["n_frames"])
    assert np.array_equal(pf, want_pf)
    assert np.array_equal(rec, want_rec), (rec, want_rec)
    assert np.array_equal(lst[:rec[0]], want_lst) and np.array_equal(slot, want_slot)
    return want_pf, want_rec


def test_lookup_and_distinct_list_7x5_with_holes(eng):
    grid = _holes_grid()
    parts = _spread_particles(1025, grid, 1, margin=2.0)
    parts[3, 0], parts[4, 1], parts[5, 0], parts[6, 1] = np.nan, np.nan, np.inf, -np.inf        # non-finite: off the map
    pf, rec = _check_lookup(eng, parts, grid)
    x, y = parts[:, 0], parts[:, 1]
    assert (x < -4.5).any() and (x > 4.5).any() and (y < -3.5).any() and (y > 3.5).any()          # outside on all four sides
    assert np.all(pf[3:7] == -1) and rec[0] >= 5 and 0 < rec[1] < 1025


def test_lookup_and_distinct_list_single_cell(eng):
    grid = dict(cell_frame=np.array([0], np.int32), origin=(0.0, 0.0), resolution=4.0, nx=1, ny=1, n_frames=1)
    pf, rec = _check_lookup(eng, _spread_particles(65, grid, 2, margin=2.0), grid)
    assert rec[0] == 1 and 0 < rec[1] < 65


@pytest.mark.parametrize("P", [63, 65536])
def test_lookup_and_distinct_list_2049_frames(eng, P):
    grid = _wide_grid()
    pf, rec = _check_lookup(eng, _spread_particles(P, grid, 3, margin=0.5), grid)
    assert rec[0] >= (2000 if P == 65536 else 30) and pf.max() > 1024           # frames on both sides of every 1024 boundary


def test_all_particles_off_the_map(eng):
    grid = _holes_grid()
    parts = _spread_particles(130, grid, 4, margin=0.0)
    parts[:, 0] += 100.0
    pf, rec = _check_lookup(eng, parts, grid)
    assert list(rec) == [0, 130, 0, 1] and np.all(pf == -1)


# ---- update ------------------------------------------------------------------------------------------------------------------------
def _update(eng, case, obs=R.UPDATE_OBS, spread=True):
    d = _dev(eng, case["particles"])
    ov = None if case["overlap"] is None else _dev(eng, case["overlap"])
    yw = None if case["yaw"] is None else _dev(eng, case["yaw"])
    r = eng.mcl_update(d, _dev(eng, case["particle_frame"]), _dev(eng, case["frame_slot"]), _dev(eng, case["frame_yaw"]), ov, yw,
                       obs["sigma_yaw"], obs["eps_yaw"], obs["overlap_min"], want_spread=spread)
    est, sp = (r[0], r[1]) if spread else (r, None)
    return d.cpu().numpy(), est.cpu().numpy(), None if sp is None else float(sp.cpu().numpy()[0])


def _check_estimate(got_parts, est, spread, on, P):
    """The eight doubles against fp64 sums over the GPU's own weight bits."""
    p = got_parts.astype(np.float64)
    w = p[:, 3]
    want, want_spread = R.estimate(got_parts, on)
    n = P + 8                                                     # P terms, plus the roundings of the quotients
    sw = np.abs(w).sum()
    assert est[0] == 0 and est[6] == want[6] and est[7] == want[7]
    assert abs(est[1] - want[1]) <= n * U52 * sw
    assert abs(est[2] - want[2]) <= 3 * n * U52 * want[2]         # (sum w)^2 / sum w^2: twice the first sum's bound plus the second's
    for k, c in ((3, p[:, 0]), (4, p[:, 1])):                     # A / B: (dA + |A / B| dB) / B
        assert abs(est[k] - want[k]) <= n * U52 * (np.abs(w * c).sum() / sw + abs(want[k]))
    res = np.hypot((w * np.sin(p[:, 2])).sum(), (w * np.cos(p[:, 2])).sum()) / sw
    assert res >= 0.1 and abs(R.angle_diff(est[5], want[5])) <= 1e-9
    # the same sums once more (P 2^-52 <= 1.5e-11 at P = 65536; the mean's own error enters in second order only)
    assert abs(spread - want_spread) <= 1e-9 * max(want_spread, 1e-3)
    print("P %d: sum w %.17g (ref %.17g), N_eff %.6f, mean (%.9f, %.9f, %.9f), spread %.6f, first max at %d, on the map %d"
          % (P, est[1], want[1], est[2], est[3], est[4], est[5], spread, est[6], est[7]))


@pytest.mark.parametrize("P", R.UPDATE_SIZES)
def test_update_matches_the_fp64_reference(eng, P):
    case = R.update_case(P)
    got, est, spread = _update(eng, case)
    want_w, on, status = R.update_weights(case, np.float64)
    assert status == 0
    dw = float(np.abs(got[:, 3] - want_w).max())
    print("P %d: weights GPU vs fp64 %.3g (allowed %.3g)" % (P, dw, WEIGHT_TOL))
    assert dw <= WEIGHT_TOL
    assert 0.5 <= got[:, 3].max() < 1.0
    assert np.array_equal(got[:, :3], case["particles"][:, :3])
    _check_estimate(got, est, spread, on, P)
    # the stated factors: a particle off the map, a NaN score, a score under the floor
    obs = R.UPDATE_OBS
    base = case["particles"][:, 3].astype(np.float64)
    ratio = got[:, 3].astype(np.float64) / base
    off = ~on
    if off.any() and on.any():
        unit = ratio[off][0] / (obs["overlap_min"] * obs["eps_yaw"])          # the common power of two (times fp32 rounding)
        assert np.allclose(ratio[off], unit * obs["overlap_min"] * obs["eps_yaw"], rtol=1e-6)
        slot = case["frame_slot"][case["particle_frame"][on]]
        nan = np.isnan(case["overlap"][slot])
        assert nan.any()
        assert np.all(ratio[on][nan] >= unit * obs["overlap_min"] * obs["eps_yaw"] * (1 - 1e-6))
        assert np.all(ratio[on][nan] <= unit * obs["overlap_min"] * (1 + 1e-6))
    again = _update(eng, case)
    assert np.array_equal(got.view(np.int32), again[0].view(np.int32)) and np.array_equal(est.view(np.int64), again[1].view(np.int64))


def test_update_without_scores_and_without_weights(eng):
    P = 130
    case = R.update_case(P)
    case.update(particle_frame=np.full(P, -1, np.int32), frame_slot=np.full(R.UPDATE_FRAMES, -1, np.int32), overlap=None, yaw=None)
    got, est, spread = _update(eng, case)                               # U = 0, NULL score buffers
    want_w, on, status = R.update_weights(case, np.float64)
    assert status == 0 and not on.any() and np.abs(got[:, 3] - want_w).max() <= WEIGHT_TOL and 0.5 <= got[:, 3].max() < 1.0
    _check_estimate(got, est, spread, on, P)
    case["particles"][:, 3] = 0.0                                       # no positive product: status 1, weights stay the products
    got, est, spread = _update(eng, case)
    assert np.all(got[:, 3] == 0.0) and list(est) == [1, 0, 0, 0, 0, 0, -1, 0] and spread == 0.0
    case = R.update_case(P)
    case["particles"][:, 3] = 0.0
    got, est, _ = _update(eng, case)
    assert np.all(got[:, 3] == 0.0) and est[0] == 1 and est[6] == -1 and est[7] == np.count_nonzero(case["particle_frame"] >= 0)


# ---- resample ----------------------------------------------------------------------------------------------------------------------
def _weight_sets(P):
    g = np.random.default_rng(3000 + P)
    one = np.zeros(P, np.float32)
    one[g.integers(0, P)] = 0.5
    third = g.uniform(0.0, 1.0, P).astype(np.float32)
    third[::3] = 0.0
    third[g.integers(0, P)] = 0.75
    odd = g.uniform(0.0, 1.0, P).astype(np.float32)
    odd[::4], odd[1::4] = np.nan, -0.5
    if P > 2:
        odd[2] = np.inf
    odd[g.integers(0, P)] = 0.625
    return {"one": one, "equal": np.full(P, 0.5, np.float32), "third_zero": third, "nan_negative": odd,
            "nothing": np.where(np.arange(P) % 2 == 0, 0.0, -1.0).astype(np.float32)}


@pytest.mark.parametrize("P,n_out", [(1, 1), (2, 3), (65, 64), (65536, 100), (1024, 1025), (65536, 65536)])
def test_resample_equals_the_integer_reference(eng, P, n_out):
    g = np.random.default_rng(P + n_out)
    for name, w in _weight_sets(P).items():
        parts = np.empty((P, 4), np.float32)
        parts[:, :3] = g.uniform(-10, 10, (P, 3))
        parts[:, 3] = w
        seed, step = 77, (3 << 32) | 5
        d = _dev(eng, parts)
        out = torch.full((n_out, 4), -7.0, dtype=torch.float32, device=eng.device)
        anc = torch.full((n_out,), -7, dtype=torch.int32, device=eng.device)
        rec = torch.full((4,), -7, dtype=torch.int32, device=eng.device)
        eng.mcl_resample(d, seed, step, n_out=n_out, out=out, ancestors=anc, record=rec)
        out, anc, rec = out.cpu().numpy(), anc.cpu().numpy(), rec.cpu().numpy()
        assert np.array_equal(d.cpu().numpy().view(np.int32), parts.view(np.int32))           # the input is not touched
        want_anc, want_rec = R.resample(w, n_out, R.resample_offset_words(seed, step))
        assert np.array_equal(rec, want_rec), (name, rec, want_rec)
        if want_anc is None:
            assert name == "nothing" and np.all(out == -7.0) and np.all(anc == -7)             # nothing but the record is written
            continue
        assert np.array_equal(anc, want_anc), name
        want_out = parts[want_anc].copy()
        want_out[:, 3] = 1.0
        assert np.array_equal(out.view(np.int32), want_out.view(np.int32)), name
        R.check_resample_properties(w, n_out, anc)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_buffers_untouched(eng):
    from overlapnet_amd import _lib
    lib, h = eng.lib, eng._h
    P, M = 16, 4
    bufs = dict(parts=torch.full((P, 4), 3.0, dtype=torch.float32, device=eng.device),
                out=torch.full((P, 4), 3.0, dtype=torch.float32, device=eng.device),
                cell=torch.zeros(4, dtype=torch.int32, device=eng.device),
                pf=torch.full((P,), 3, dtype=torch.int32, device=eng.device),
                slot=torch.full((M,), 3, dtype=torch.int32, device=eng.device),
                lst=torch.full((M,), 3, dtype=torch.int32, device=eng.device),
                rec=torch.full((8,), 3, dtype=torch.int32, device=eng.device),
                psi=torch.zeros(M, dtype=torch.float32, device=eng.device),
                ov=torch.full((M,), 0.5, dtype=torch.float32, device=eng.device),
                yw=torch.zeros(M, dtype=torch.int32, device=eng.device),
                est=torch.full((10,), 3.0, dtype=torch.float64, device=eng.device),
                anc=torch.full((P,), 3, dtype=torch.int32, device=eng.device))
    before = {k: v.clone() for k, v in bufs.items()}
    p = {k: C.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    rec4 = C.c_void_p(bufs["rec"].data_ptr() + 4)                         # not 16-byte aligned
    est8 = C.c_void_p(bufs["est"].data_ptr() + 8)
    parts4 = C.c_void_p(bufs["parts"].data_ptr() + 4)
    st = eng._stream()

    def predict(parts=p["parts"], n=P, res=1.0, nx=2, ny=2, m=M, cell=p["cell"], pf=p["pf"], slot=p["slot"], lst=p["lst"], rec=p["rec"]):
        return lib.ovn_mcl_predict(h, parts, n, 0.1, 0.0, 0.0, 0.1, 0.1, 0.1, 1, 2, cell, 0.0, 0.0, res, nx, ny, m, pf, slot, lst, rec, st)

    def update(parts=p["parts"], n=P, m=M, u=M, sig=10.0, eps=0.1, omin=0.05, pf=p["pf"], slot=p["slot"], psi=p["psi"], ov=p["ov"],
               yw=p["yw"], est=p["est"]):
        return lib.ovn_mcl_update(h, parts, n, pf, slot, psi, m, ov, yw, u, sig, eps, omin, est, None, st)

    def resample(parts=p["parts"], n=P, out=p["out"], n_out=P, anc=p["anc"], rec=p["rec"]):
        return lib.ovn_mcl_resample(h, parts, n, 1, 2, out, n_out, anc, rec, st)

    bad = [predict(n=0), predict(n=65537), predict(nx=0), predict(ny=-1), predict(nx=65536, ny=32768), predict(m=0), predict(res=0.0),
           predict(res=-1.0), predict(res=float("nan")), predict(parts=None), predict(cell=None), predict(pf=None), predict(slot=None),
           predict(lst=None), predict(rec=None), predict(rec=rec4), predict(parts=parts4),
           update(n=0), update(n=65537), update(m=0), update(u=-1), update(u=M + 1), update(sig=0.0), update(sig=float("nan")),
           update(omin=0.0), update(omin=-0.1), update(eps=-0.01), update(eps=1.01), update(eps=float("nan")), update(parts=None),
           update(pf=None), update(slot=None), update(psi=None), update(ov=None), update(yw=None), update(est=None), update(est=est8),
           resample(n=0), resample(n=65537), resample(n_out=0), resample(n_out=65537), resample(parts=None), resample(out=None),
           resample(anc=None), resample(rec=None), resample(rec=rec4), resample(out=p["parts"]),
           resample(out=C.c_void_p(bufs["parts"].data_ptr() + 16 * (P - 1)))]
    assert bad == [1] * len(bad), bad
    assert lib.ovn_last_error()
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), k
    # the engine's own checks: shapes, dtypes, devices
    with pytest.raises(_lib.OvnError):
        eng.mcl_predict(bufs["parts"][:, :3], (0, 0, 0), (0, 0, 0), 0, 0, bufs["cell"], (0, 0), 1.0, 2, 2, M)
    with pytest.raises(_lib.OvnError):
        eng.mcl_predict(bufs["parts"], (0, 0, 0), (0, 0, 0), 0, 0, bufs["cell"], (0, 0), 1.0, 3, 2, M)      # 6 cells, 4 entries
    with pytest.raises(_lib.OvnError):
        eng.mcl_update(bufs["parts"], bufs["pf"], bufs["slot"], bufs["psi"], bufs["ov"], None, 10.0, 0.1, 0.05)
    with pytest.raises(_lib.OvnError):
        eng.mcl_resample(bufs["parts"], 0, 0, out=bufs["parts"])
    with pytest.raises(_lib.OvnError):
        eng.mcl_resample(bufs["parts"].cpu(), 0, 0)


# ---- the localizer -----------------------------------------------------------------------------------------------------------------
MAP_POSES = np.array([[3.0 * k, 0.5 * (k % 2), 0.3 * k - 0.6] for k in range(6)])


def _moved(points, pose):
    """The scan `points` as a sensor at world pose (x, y, heading) would see it if the fixture scan was taken at the world origin."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    out = np.array(points, np.float32).reshape(-1, 4).copy()
    d = out[:, :2].astype(np.float64) - pose[:2]
    out[:, 0], out[:, 1] = c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]
    return out


@pytest.fixture(scope="module")
def world(fixture_npz, tmp_path_factory):
    from tools import synthetic as S
    from overlapnet_amd.infer import Infer
    from overlapnet_amd.localization import OverlapMap
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07",
           "data_root_folder": str(tmp_path_factory.mktemp("mcl")), "use_depth": True, "use_normals": True,
           "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16,
           "pretrained_weightsfilename": ""}
    infer = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    clouds = [_moved(fixture_npz["points_0"], p) for p in MAP_POSES]
    mp = OverlapMap(infer, None, MAP_POSES, resolution=1.0, scans=clouds)
    yield dict(infer=infer, map=mp, clouds=clouds)
    infer.close()


def test_map_is_cached_and_gridded(world):
    mp = world["map"]
    assert len(world["infer"].feature_volumes) == 6 and mp.n_frames == 6
    table = mp.cell_frame.cpu().numpy()
    assert np.array_equal(table, mp.cell_frame_host) and set(np.unique(table)) == {-1, 0, 1, 2, 3, 4, 5}
    from overlapnet_amd.localization import cell_of
    own = cell_of(MAP_POSES[:, 0], MAP_POSES[:, 1], mp.origin_x, mp.origin_y, mp.resolution, mp.nx, mp.ny)
    assert np.array_equal(table[own], np.arange(6))                      # a frame's own cell names it
    assert np.array_equal(mp.occupied_cells, np.nonzero(table >= 0)[0])


def test_step_equals_the_stages_chained_by_hand(world):
    from overlapnet_amd.localization import MonteCarloLocalizer, _features_of
    mp, infer, eng = world["map"], world["infer"], world["infer"].engine
    kw = dict(seed=5, resample_fraction=1.0)
    a, b, c = (MonteCarloLocalizer(mp, 256, **kw) for _ in range(3))
    for loc in (a, b, c):
        loc.init_around((7.0, 0.2, 0.4), (3.0, 0.6, 0.5))
    assert np.array_equal(a.particles.cpu().numpy(), b.particles.cpu().numpy())
    cache = infer.feature_volumes
    hand = c.particles.clone()
    drive = [(world["clouds"][2], (0.5, 0.0, 0.02)), (world["clouds"][3], (0.6, 0.1, -0.03))]
    sigma = (0.2, 0.1, 0.05)
    for step, (scan, odom) in enumerate(drive):
        ea, eb = a.step(scan, odom, sigma), b.step(scan, odom, sigma)
        assert ea == eb and np.array_equal(a.particles.cpu().numpy().view(np.int32), b.particles.cpu().numpy().view(np.int32))
        # by hand: leg, predict, the record, the sweep over the listed frames, update, resample
        q = _features_of(infer, scan)
        pf, slot, lst, rec = eng.mcl_predict(hand, odom, sigma, 5, step, mp.cell_frame, (mp.origin_x, mp.origin_y), mp.resolution, mp.nx,
                                             mp.ny, 6)
        u, off = (int(v) for v in rec.cpu().numpy()[:2])
        assert (ea.frames_scored, ea.off_map) == (u, off) and u >= 2
        assert np.array_equal(a.last["frame_list"].cpu().numpy(), lst[:u].cpu().numpy())
        r = eng.heads(cache.device_features, q, lidx=lst[:u], n=u, spec_l=cache.device_spectra, spec_r=eng.spectrum(q),
                      dcache_l=cache.device_delta_cache)
        assert torch.equal(a.last["overlap"], r["overlap"]) and torch.equal(a.last["yaw"], r["yaw"])
        est = eng.mcl_update(hand, pf, slot, mp.frame_yaw, r["overlap"], r["yaw"], a.sigma_yaw, a.eps_yaw, a.overlap_min)
        est = est.cpu().numpy()
        parts = hand.cpu().numpy()
        on = pf.cpu().numpy() >= 0
        _check_estimate(parts, a.last["estimate"], R.estimate(parts, on)[1], on, 256)      # (no spread asked for: the reference's own)
        assert np.array_equal(a.last["estimate"].view(np.int64), est.view(np.int64))
        assert (ea.x, ea.y, ea.yaw, ea.n_eff) == (est[3], est[4], est[5], est[2]) and not ea.lost
        assert ea.resampled == (est[2] < 256)
        if ea.resampled:
            out, anc, rrec = eng.mcl_resample(hand, 5, step)
            assert list(rrec.cpu().numpy()) == [0, 256, 0, 1]
            assert np.array_equal(a.last["ancestors"].cpu().numpy(), anc.cpu().numpy())
            want_anc, _ = R.resample(parts[:, 3], 256, R.resample_offset_words(5, step))
            assert np.array_equal(anc.cpu().numpy(), want_anc)
            hand = out
        assert np.array_equal(a.particles.cpu().numpy().view(np.int32), hand.cpu().numpy().view(np.int32))
    assert ea.resampled                                                  # the ping-pong buffers were exercised


def test_heading_comes_from_the_yaw_head(world):
    """The query is map frame 3's own scan: the correlation of a volume with itself peaks at zero shift whatever the weights, so the
    network's yaw is 0 and the filter must turn the particles in that frame's cell towards the frame's heading."""
    from overlapnet_amd.localization import MonteCarloLocalizer
    mp = world["map"]
    f, P = 3, 512
    loc = MonteCarloLocalizer(mp, P, seed=1, resample_fraction=0.0)
    loc.init_around((MAP_POSES[f, 0], MAP_POSES[f, 1], 0.0), (0.0, 0.0, 0.0))
    headings = (-np.pi + 2 * np.pi * (np.arange(P) + 1.0) / P).astype(np.float32)
    loc.particles[:, 2] = torch.from_numpy(headings).to(loc.particles.device)
    e = loc.step(world["clouds"][f], (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert e.frames_scored == 1 and e.off_map == 0 and not e.lost and not e.resampled
    assert int(loc.last["frame_list"].cpu().numpy()[0]) == f and int(loc.last["yaw"].cpu().numpy()[0]) == 0
    psi = MAP_POSES[f, 2]
    spacing = 360.0 / P
    mean_err = abs(np.degrees(R.angle_diff(e.yaw, psi)))
    best = int(loc.last["estimate"][6])
    best_err = abs(np.degrees(R.angle_diff(headings[best], psi)))
    print("circular mean %.4f deg from the frame's heading (sigma_yaw %.1f), best particle %.4f deg (spacing %.3f)"
          % (mean_err, loc.sigma_yaw, best_err, spacing))
    assert mean_err <= loc.sigma_yaw and best_err <= 1.0 + spacing
    assert abs(e.x - MAP_POSES[f, 0]) < 1e-5 and abs(e.y - MAP_POSES[f, 1]) < 1e-5


def test_sharded_infer_is_refused(world):
    from overlapnet_amd import _lib
    from overlapnet_amd.localization import OverlapMap

    class Sharded(object):
        _world = 2
    with pytest.raises(_lib.OvnError, match="sharded"):
        OverlapMap(Sharded(), None, MAP_POSES, 1.0, scans=world["clouds"])


def test_converged_filter_shrinks_and_a_lost_one_starts_over(world):
    from overlapnet_amd.localization import MonteCarloLocalizer
    mp = world["map"]
    loc = MonteCarloLocalizer(mp, 300, seed=2, resample_fraction=1.0, converged_particles=70, converge_radius=1e9)
    loc.init_around((MAP_POSES[2, 0], MAP_POSES[2, 1], MAP_POSES[2, 2]), (0.3, 0.3, 0.2))
    e = loc.step(world["clouds"][2], (0.0, 0.0, 0.0), (0.05, 0.05, 0.01))
    assert e.resampled and not e.lost and tuple(loc.particles.shape) == (70, 4)          # spread < radius: down to 70
    assert torch.all(loc.particles[:, 3] == 1.0) and int(loc.last["ancestors"].max()) < 300
    e = loc.step(world["clouds"][2], (0.0, 0.0, 0.0), (0.05, 0.05, 0.01))                # the next step runs on the 70
    assert e.off_map <= 70 and tuple(loc.particles.shape) == (70, 4) and np.isfinite([e.x, e.y, e.yaw, e.n_eff]).all()
    loc.init_around((1000.0, 1000.0, 0.0), (0.1, 0.1, 0.1))                             # nowhere near the map
    e = loc.step(world["clouds"][2], (0.0, 0.0, 0.0), (0.05, 0.05, 0.01))
    assert e.lost and e.frames_scored == 0 and e.off_map == 300 and not e.resampled
    assert tuple(loc.particles.shape) == (300, 4)                                         # init_uniform ran: back on the map
    cells = loc.map.cell_frame_host
    from overlapnet_amd.localization import cell_of
    p = loc.particles.cpu().numpy()
    c = cell_of(p[:, 0], p[:, 1], mp.origin_x, mp.origin_y, mp.resolution, mp.nx, mp.ny)
    assert np.all(c >= 0) and np.all(cells[c] >= 0)
