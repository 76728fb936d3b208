"""GPU (MI355X): `ovn_icp_register` (csrc/icp_register.hip) against the fp64 NumPy statement of the same algorithm
(tests/_icp_ref.py), which is given the maps the GPU projected, copied back -- only the ICP is compared.

Tolerance of the pose comparisons.  The kernel's per-point arithmetic is fp32, the reference's fp64.  How far that moves the result is
measured on the reference itself: `register(arith=np.float32)` against `register()` on the cases below ends at most 1.72e-5 m and
1.55e-4 deg apart (real scan, case 4: one association flips; every other case, real or room, <= 4e-7 m and 2e-6 deg).  The GPU is
allowed ten times that figure, for a different atan2f / asinf and another summation order: POSE_TOL."""
import os

import numpy as np
import pytest
import torch

import _icp_ref as R
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

F32_FIGURE = (1.8e-5, 1.6e-4)                              # [m], [deg]: the reference in float32 against itself in fp64, rounded up
POSE_TOL = (10 * F32_FIGURE[0], 10 * F32_FIGURE[1])
# a pose that far away moves a residual by at most |dt| + |dr| * max_range: the bound on |rms - rms_ref|
RMS_TOL = POSE_TOL[0] + np.radians(POSE_TOL[1]) * 50.0
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


def _project(eng, clouds, H, W):
    from overlapnet_amd import preprocess as P
    r = P.project_scans(clouds, engine=eng, proj_H=H, proj_W=W, want=("range", "vertex", "normal"))
    return r["vertex"], r["normal"], r["range"]


def _host(maps, i):
    v, n, r = maps
    return r[i].cpu().numpy(), v[i].cpu().numpy(), n[i].cpu().numpy()


def _run(eng, maps, pairs, init, **kw):
    dev = eng.device
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    src = torch.from_numpy(np.ascontiguousarray(pairs[:, 0])).to(dev)
    tgt = torch.from_numpy(np.ascontiguousarray(pairs[:, 1])).to(dev)
    T0 = torch.from_numpy(np.ascontiguousarray(np.asarray(init, np.float64).reshape(-1, 4, 4))).to(dev)
    return eng.icp_register(maps[0], maps[1], maps[2], src, tgt, T0, **kw)


@pytest.fixture(scope="module")
def real(eng, fixture_npz):
    """Scans 0: points_0 (the target), 1: points_1, 2..5: points_0 moved by inv(T_gt) of REAL_CASES; the GPU's maps, their host
    copies, and the reference's registrations (computed once)."""
    clouds = [fixture_npz["points_0"], fixture_npz["points_1"]]
    gts, inits = [], []
    for yaw, t, off in R.REAL_CASES:
        T_gt = R.make_pose(yaw, t)
        clouds.append(R.moved_cloud(fixture_npz["points_0"], np.linalg.inv(T_gt)))
        gts.append(T_gt)
        inits.append(R.rz(yaw + off))
    maps = _project(eng, clouds, 64, 900)
    host = [_host(maps, i) for i in range(len(clouds))]
    pairs = [(2 + k, 0) for k in range(4)] + [(1, 0)]
    inits.append(np.eye(4))
    refs = [R.register(host[s], host[t], T0) for (s, t), T0 in zip(pairs, inits)]
    return dict(maps=maps, host=host, pairs=pairs, inits=inits, gts=gts, refs=refs)


def _compare(tag, pose, stats, ref):
    dt, dr = R.pose_error(pose, ref["pose"])
    print("%s: GPU vs reference %.3g m %.3g deg (allowed %.3g / %.3g); inliers %d vs %d, rms %.6f vs %.6f, last step %.2g m %.2g rad"
          % (tag, dt, dr, POSE_TOL[0], POSE_TOL[1], stats[2], ref["inliers"], stats[4], ref["rms"], stats[5], stats[6]))
    assert np.all(np.isfinite(pose)) and np.all(np.isfinite(stats))
    assert stats[0] == ref["status"] == 0 and stats[1] == ref["solved"] and stats[3] == ref["valid"]
    assert np.array_equal(pose[3], [0, 0, 0, 1])
    assert dt <= POSE_TOL[0] and dr <= POSE_TOL[1]
    assert abs(stats[4] - ref["rms"]) <= RMS_TOL


def test_recovers_a_moved_real_scan_like_the_reference(eng, real):
    pose, stats = _run(eng, real["maps"], real["pairs"], real["inits"])
    pose, stats = pose.cpu().numpy(), stats.cpu().numpy()
    for k in range(4):
        _compare("case %d %s" % (k, R.REAL_CASES[k]), pose[k], stats[k], real["refs"][k])
        dt, dr = R.pose_error(pose[k], real["gts"][k])
        print("   from the ground truth: %.2f mm %.4f deg" % (1e3 * dt, dr))
        assert dt <= 5.0e-3 and dr <= 0.01                       # the reference ends 0.8 / 1.7 / 1.7 / 4.6 mm, <= 0.006 deg away
        assert 16000 <= stats[k][2] <= 28000
    # points_1 -> points_0 from the identity: 0.68 m of forward motion, 24 330 inliers, rms 0.027 in the reference
    _compare("points_1 -> points_0", pose[4], stats[4], real["refs"][4])
    ref = real["refs"][4]
    assert abs(ref["pose"][0, 3] - 0.68) < 0.01 and abs(ref["inliers"] - 24330) <= 5 and abs(ref["rms"] - 0.027) < 1e-3
    assert abs(stats[4][2] - ref["inliers"]) <= 0.01 * ref["valid"]      # at most the ambiguous share the next test allows


def _ambiguous(d, max_range=50.0, max_dist=2.0, cos_min=0.8):
    """Source pixels whose association or gate the fp32 kernel may legitimately decide differently from the fp64 reference: the fp64
    pixel coordinate within 1e-3 px of a pixel border, or a gate value within 1e-4 (relative) of its threshold.  -> (all of them,
    the border part, the `hard` ones: near a gate, or near a border in both directions)."""
    frac = lambda a: np.abs(a - np.round(a))
    bu, bv = frac(d["uf"]) <= 1e-3, frac(d["vf"]) <= 1e-3
    dist = np.sqrt(d["dist2"])
    gate = ((np.abs(d["d"] - max_range) <= 1e-4 * max_range) | (np.abs(dist - max_dist) <= 1e-4 * max_dist)
            | (np.abs(d["cosv"] - cos_min) <= 1e-4 * cos_min))
    fin = np.isfinite(d["d"])
    return fin & (bu | bv | gate), fin & (bu | bv), fin & (gate | (bu & bv))


def _system_bounds(d, alts, amb, hard, huber=0.2):
    """Entry-wise bounds on |A - A_ref| (21) and |b - b_ref| (6), computed from the reference.
    A point on a pixel border may take the pixel next to its own instead: it loses the row it has and gains that pixel's, at most
    |K_own| + max over the four neighbours |K_neighbour| (K: _icp_ref.one_pass, the row whether or not the gates pass).
    A `hard` point (near a gate, or in a pixel corner) gets the bound that holds for any row: J = [n, p' x n] with |n| = 1, so
    |J_k| <= c_k = (1, 1, 1, |p'|, |p'|, |p'|), and w |r| <= huber: 2 c_k c_l and 2 c_k huber.
    Every other row carries fp32 rounding: a component of p' = R p + t is off by at most 6 eps |p'| (R and t rounded to fp32, three
    products, three sums), so r = n . (p' - q) by at most sqrt(3) 6 eps |p'| <= 12 eps |p'|, J_k by at most 12 eps c_k (the cross
    product adds its own three roundings), and w = huber / |r| by 12 eps |p'| / huber."""
    dd = np.where(np.isfinite(d["d"]), d["d"], 0.0)
    c = np.stack([np.ones_like(dd)] * 3 + [dd] * 3, axis=1)
    soft = amb & ~hard
    altA = np.max([np.abs(a["KA"][soft]) for a in alts], axis=0)
    altb = np.max([np.abs(a["Kb"][soft]) for a in alts], axis=0)
    tolA = (np.abs(d["KA"][soft]) + altA).sum(axis=0)
    tolb = (np.abs(d["Kb"][soft]) + altb).sum(axis=0)
    ch, co, do = c[hard], c[d["ok"] & ~amb], dd[d["ok"] & ~amb]
    tolA = tolA + np.array([2.0 * (ch[:, i] * ch[:, j]).sum() + (co[:, i] * co[:, j] * (24 * EPS + 12 * EPS * do / huber)).sum()
                            for i, j in R.TRI])
    tolb = tolb + np.array([2.0 * huber * ch[:, k].sum() + (co[:, k] * (12 * EPS * do + 12 * EPS * huber)).sum() for k in range(6)])
    return tolA, tolb


SHIFTS = ((-1, 0), (1, 0), (0, -1), (0, 1))


def test_first_pass_normal_equations_match_the_reference(eng, real):
    _, _, system = _run(eng, real["maps"], real["pairs"], real["inits"], want_system=True)
    system = system.cpu().numpy()
    diag = [0, 6, 11, 15, 18, 20]
    for k, ((s, t), T0) in enumerate(zip(real["pairs"], real["inits"])):
        d = R.one_pass(real["host"][s], real["host"][t], T0, detail=True)
        alts = [R.one_pass(real["host"][s], real["host"][t], T0, detail=True, shift=sh) for sh in SHIFTS]
        ref = R.system_vector(d)
        amb, border, hard = _ambiguous(d)
        n_amb, valid = int(amb.sum()), d["valid"]
        tolA, tolb = _system_bounds(d, alts, amb, hard)
        errA, errb = np.abs(system[k][:21] - ref[:21]), np.abs(system[k][21:27] - ref[21:27])
        print("pair %d: count %d vs %d; ambiguous %d of %d valid (%.2f %%, border alone %.2f %%, hard %d); max |dA| / bound %.3g, "
              "max |db| / bound %.3g; bound / |A_kk| %s" % (k, system[k][27], ref[27], n_amb, valid, 100.0 * n_amb / valid,
                                                          100.0 * border.sum() / valid, hard.sum(), (errA / tolA).max(),
                                                          (errb / tolb).max(),
                                                          np.array2string(tolA[diag] / np.abs(ref[diag]), precision=3)))
        assert np.all(np.isfinite(system[k]))
        assert n_amb <= 0.01 * valid                              # a condition on the case, not a tolerance
        assert abs(system[k][27] - ref[27]) <= n_amb
        assert np.all(errA <= tolA) and np.all(errb <= tolb)


def test_first_pass_without_ambiguous_pixels_matches_to_rounding(eng, real):
    """The sharp form of the test above.  Every source pixel adds its row on its own, so the ambiguous ones can be taken out of
    the input: their range set to -1 in a copy of the source scan.  What is left has no pixel near a border or a gate, the kernel
    and the reference must then make the same associations -- equal counts -- and A and b may differ by fp32 rounding alone
    (`_system_bounds` without ambiguous points: a worst-case sum, about 1e-4 of A's diagonal)."""
    v, n, r = real["maps"]
    base = r.shape[0]
    cut, pairs = [], []
    for k, ((s, t), T0) in enumerate(zip(real["pairs"], real["inits"])):
        d = R.one_pass(real["host"][s], real["host"][t], T0, detail=True)
        amb, _, _ = _ambiguous(d)
        rs = real["host"][s][0].copy()
        rs.reshape(-1)[d["sel"][amb]] = -1.0
        cut.append(rs)
        pairs.append((base + k, t))
    src = [s for s, _ in real["pairs"]]
    maps = (torch.cat([v, v[src]]), torch.cat([n, n[src]]), torch.cat([r, torch.from_numpy(np.stack(cut)).to(r.device)]))
    _, _, system = _run(eng, maps, pairs, real["inits"], want_system=True)
    system = system.cpu().numpy()
    diag = [0, 6, 11, 15, 18, 20]
    for k, ((s, t), T0) in enumerate(zip(real["pairs"], real["inits"])):
        d = R.one_pass((cut[k],) + real["host"][s][1:], real["host"][t], T0, detail=True)
        amb, _, _ = _ambiguous(d)
        assert not amb.any()
        ref = R.system_vector(d)
        none = np.zeros_like(amb)
        tolA, tolb = _system_bounds(d, [d], none, none)
        errA, errb = np.abs(system[k][:21] - ref[:21]), np.abs(system[k][21:27] - ref[21:27])
        print("pair %d without its ambiguous pixels: count %d vs %d; max |dA| / rounding bound %.3g, max |db| / rounding bound %.3g; "
              "bound / |A_kk| %s" % (k, system[k][27], ref[27], (errA / tolA).max(), (errb / tolb).max(),
                                    np.array2string(tolA[diag] / np.abs(ref[diag]), precision=2)))
        assert system[k][27] == ref[27]
        assert np.all(errA <= tolA) and np.all(errb <= tolb)


@pytest.mark.parametrize("shape", R.ROOM_SHAPES + [R.ODD_ROOM_SHAPE])
def test_small_shapes_in_the_box_room(eng, shape):
    """16 x 100; 8 x 90 (720 pixels: no multiple of 64; 180 four-pixel groups, fewer than the 512 threads); 17 x 131 (2227 pixels: no
    multiple of 4, so the scalar loads and a last group of 3 pixels, and 557 groups: a second stride for 45 threads)."""
    H, W = shape
    clouds, pairs, inits = [], [], []
    for k, case in enumerate(R.ROOM_CASES):
        tc, sc, T_gt, T0 = R.room_pair(case)
        clouds += [tc, sc]
        pairs.append((2 * k + 1, 2 * k))
        inits.append(T0)
    maps = _project(eng, clouds, H, W)
    pose, stats = _run(eng, maps, pairs, inits)
    pose, stats = pose.cpu().numpy(), stats.cpu().numpy()
    for k, (s, t) in enumerate(pairs):
        ref = R.register(_host(maps, s), _host(maps, t), inits[k])
        _compare("%dx%d %s" % (H, W, R.ROOM_CASES[k]), pose[k], stats[k], ref)
        assert abs(stats[k][2] - ref["inliers"]) <= 0.01 * ref["valid"] and ref["inliers"] >= 500
    if (H * W) % 4 == 0:
        # the same maps 4 bytes into their allocations: not 16-byte aligned, so the scalar loads walk the same groups
        off = [torch.cat([m.new_zeros(1), m.reshape(-1)])[1:].reshape(m.shape) for m in maps]
        assert all(o.data_ptr() % 16 == 4 and o.is_contiguous() for o in off)
        pose2, stats2 = _run(eng, off, pairs, inits)
        # the same groups in the same order, the same arithmetic: the same bits
        assert torch.equal(torch.from_numpy(pose).to(pose2.device), pose2) and torch.equal(torch.from_numpy(stats).to(stats2.device), stats2)
        for k, (s, t) in enumerate(pairs):
            _compare("%dx%d unaligned %s" % (H, W, R.ROOM_CASES[k]), pose2[k].cpu().numpy(), stats2[k].cpu().numpy(),
                     R.register(_host(maps, s), _host(maps, t), inits[k]))


def test_degenerate_pairs(eng):
    from overlapnet_amd._lib import OvnError
    H, W = 8, 90
    tc, sc, _, T0 = R.room_pair(R.ROOM_CASES[0])
    v, n, r = (t.clone() for t in _project(eng, [tc, sc, tc, tc], H, W))
    v[2], n[2], r[2] = -1.0, -1.0, -1.0                    # scan 2: all empty
    n[3] = -1.0                                            # scan 3: a target without a single valid normal
    maps = (v, n, r)
    T0 = T0.copy()
    T0[:3, 3] = [0.05, -0.03, 0.01]                        # nothing special about its bits
    pairs = [(2, 0), (1, 3), (4, 0), (1, -1), (1, 0)]
    pose, stats, system = _run(eng, maps, pairs, [T0] * 5, want_system=True)
    T0d = torch.from_numpy(T0).to(eng.device)
    assert bool(torch.isfinite(pose).all()) and bool(torch.isfinite(stats).all()) and bool(torch.isfinite(system).all())
    st = stats.cpu().numpy()
    for k in (0, 1):                                       # empty source; target without normals
        assert torch.equal(pose[k], T0d) and st[k][0] == 1 and st[k][1] == 0 and st[k][2] == 0 and st[k][4] == 0
    assert st[0][3] == 0 and st[1][3] == int((r[1] > 0).sum())
    for k in (2, 3):                                       # an index out of range
        assert torch.equal(pose[k], T0d) and st[k][0] == 2 and not st[k][1:].any() and not system[k].cpu().numpy().any()
    assert st[4][0] == 0 and st[4][1] == 20 and not torch.equal(pose[4], T0d)

    # iterations = 0: T0 back, with the statistics of the one pass at T0
    p0, s0 = _run(eng, maps, [(1, 0)], [T0], iterations=0)
    d = R.one_pass(_host(maps, 1), _host(maps, 0), T0, detail=True)
    amb, _, _ = _ambiguous(d)
    s0 = s0.cpu().numpy()[0]
    print("iterations=0: inliers %d vs %d (ambiguous %d), rms %.6f vs %.6f" % (s0[2], d["count"], amb.sum(), s0[4], np.sqrt(d["e"] / d["count"])))
    assert torch.equal(p0[0], T0d) and s0[0] == 0 and s0[1] == 0 and s0[5] == 0 and s0[6] == 0 and s0[3] == d["valid"]
    assert abs(s0[2] - d["count"]) <= amb.sum()
    if amb.sum() == 0:
        assert abs(s0[4] - np.sqrt(d["e"] / d["count"])) <= 12 * EPS * 50.0     # fp32 rounding of a residual at <= 50 m (_system_bounds)

    # a T0 that holds a NaN matches no point: it comes back as it is, status 1, finite statistics
    Tn = T0.copy()
    Tn[0, 3] = np.nan
    pn, sn = _run(eng, maps, [(1, 0)], [Tn])
    sn = sn.cpu().numpy()[0]
    assert np.array_equal(pn[0].cpu().numpy(), Tn, equal_nan=True) and sn[0] == 1 and sn[1] == 0 and sn[2] == 0 and np.all(np.isfinite(sn))

    # no pairs: nothing to do
    pe, se = _run(eng, maps, np.zeros((0, 2), np.int32), np.zeros((0, 4, 4)))
    assert tuple(pe.shape) == (0, 4, 4) and tuple(se.shape) == (0, 8)
    # argument errors
    for bad in (dict(iterations=-1), dict(iterations=1001), dict(max_dist=0.0), dict(cos_min=-0.5), dict(huber=0.0)):
        with pytest.raises(OvnError):
            _run(eng, maps, [(1, 0)], [T0], **bad)
    with pytest.raises(OvnError, match="contiguous"):
        eng.icp_register(v, n, r.double(), torch.zeros(1, dtype=torch.int32, device=eng.device),
                         torch.zeros(1, dtype=torch.int32, device=eng.device), T0d.reshape(1, 4, 4))


def test_a_pair_has_the_same_bits_alone_and_in_any_batch(eng, real):
    pairs = [(2, 0), (3, 0), (4, 0), (5, 0), (1, 0), (0, 1), (2, 1)]
    inits = real["inits"][:5] + [np.eye(4), R.rz(30.0)]
    a = _run(eng, real["maps"], pairs, inits, want_system=True)
    b = _run(eng, real["maps"], pairs, inits, want_system=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)                               # run after run
    c = _run(eng, real["maps"], pairs[::-1], inits[::-1], want_system=True)
    for x, y in zip(a, c):
        assert torch.equal(x, y.flip(0))                       # at any position
    for k in range(len(pairs)):
        one = _run(eng, real["maps"], [pairs[k]], [inits[k]], want_system=True)
        for x, y in zip(a, one):
            assert torch.equal(x[k], y[0]), (k, pairs[k])      # alone
    assert len({a[0][k].cpu().numpy().tobytes() for k in range(len(pairs))}) == len(pairs)     # seven different results


def test_infer_verify_top_k(tmp_path, fixture_npz):
    from overlapnet_amd.infer import Infer
    from overlapnet_amd import registration as G
    scans = tmp_path / "scans"
    os.makedirs(scans)
    moves = [(0.0, (0, 0, 0)), (5.0, (0.5, 0.1, 0.0)), (-8.0, (1.0, -0.3, 0.02)), (3.0, (0.4, 0.2, 0.0))]
    clouds = [R.moved_cloud(fixture_npz["points_%d" % (i % 2)], np.linalg.inv(R.make_pose(*m))) for i, m in enumerate(moves)]
    for i, c in enumerate(clouds):
        c.tofile(scans / ("%06d.bin" % i))
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(tmp_path),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": ""}
    w = S.make_test_weights(4, seed=0)
    inf = Infer(dict(cfg, scan_folder=str(scans)), weights=w)
    inf.cache_frames(3)
    got = inf.verify_top_k(3, [0, 1, 2], k=3, overlap_thres=None)
    assert len(got) == 3 and sorted(g[0] for g in got) == [0, 1, 2]
    assert [g[1] for g in got] == sorted((g[1] for g in got), reverse=True)
    assert all(g[6] is None for g in got)
    # the same pairs through register_scans: candidate -> current frame, seeded with Rz(-yaw degrees) stated on its own
    regs = G.register_scans(inf.engine, [clouds[3]] + [clouds[g[0]] for g in got], [(i + 1, 0) for i in range(3)],
                            [R.rz(-g[2]) for g in got])
    for g, r in zip(got, regs):
        print("frame %d overlap %.3f yaw %d: fitness %.3f rms %.4f status %d" % (g[0], g[1], g[2], r.fitness, r.rms, r.status))
        assert np.array_equal(g[3], r.pose) and g[4] == r.fitness and g[5] == r.rms
        assert g[3].shape == (4, 4) and np.all(np.isfinite(g[3])) and 0.0 <= g[4] <= 1.0
    fit = sorted(r.fitness for r in regs)
    thr = 0.5 * (fit[0] + fit[1]) if fit[0] < fit[1] else fit[0] + 1.0
    acc = inf.verify_top_k(3, [0, 1, 2], k=3, overlap_thres=None, min_fitness=thr)
    assert [a[6] for a in acc] == [bool(r.status == 0 and r.fitness >= thr) for r in regs]
    acc = inf.verify_top_k(3, [0, 1, 2], k=3, overlap_thres=None, max_rms=0.0)
    assert [a[6] for a in acc] == [bool(r.status == 0 and r.rms <= 0.0) for r in regs]
    acc = inf.verify_top_k(3, [0, 1, 2], k=3, overlap_thres=None, min_fitness=0.0, max_rms=1e9, iterations=5)
    assert all(isinstance(a[6], bool) for a in acc)
    assert inf.verify_top_k(3, [], k=3) == []
    inf.close()
    plain = Infer(cfg, weights=w)
    with pytest.raises(ValueError, match="scan_folder"):
        plain.verify_top_k(3, [0, 1, 2])
    plain.close()


def test_verify_top_k_recovers_rotations_from_the_networks_yaw(tmp_path, fixture_npz):
    """The whole chain on the GPU, no trained weights needed: the correlation head is a shift detector whatever its weights, so for
    candidates that are the current scan rotated about z, `infer_top_k`'s yaw has the sign (and, through the leg's 900 -> 360
    columns, roughly the size) of the rotation.  Candidate i is the base scan turned by cols_i image columns (0.4 degrees each), the
    current frame by 25: the pose candidate -> current is Rz((25 - cols_i) 0.4 degrees) exactly, no translation.  `verify_top_k`
    must seed with Rz(-yaw) and end there; with Rz(+yaw) or with the yaw read as a bin the ICP ends degrees away.
    Bounds: the reference recovers the moved real scan to <= 5 mm and 0.01 degrees (tests/test_icp_host.py); here source and target
    are the same points, so the same bounds hold with room to spare."""
    from overlapnet_amd.infer import Infer
    scans = tmp_path / "scans"
    os.makedirs(scans)
    cols = [0, 50, -115, 25]
    for i, c in enumerate(cols):
        S.z_rotated(fixture_npz["points_0"], c).tofile(scans / ("%06d.bin" % i))
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07", "data_root_folder": str(tmp_path),
           "use_depth": True, "use_normals": True, "use_class_probabilities": False, "use_class_probabilities_pca": False,
           "use_intensity": False, "batch_size": 16, "pretrained_weightsfilename": "", "scan_folder": str(scans)}
    inf = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    inf.cache_frames(3)
    got = inf.verify_top_k(3, [0, 1, 2], k=3, overlap_thres=None, min_fitness=0.8, max_rms=0.01)
    assert sorted(g[0] for g in got) == [0, 1, 2]
    for fid, ov, yaw, pose, fitness, rms, accepted in got:
        truth = (cols[3] - cols[fid]) * 0.4
        dt, dr = R.pose_error(pose, R.rz(truth))
        print("frame %d: yaw %d, truth %.1f deg, ends %.2g m %.2g deg away, fitness %.3f rms %.2g" % (fid, yaw, truth, dt, dr, fitness, rms))
        assert yaw * truth < 0                                    # the network's yaw turns the other way: current into reference
        assert dt <= 5.0e-3 and dr <= 0.01 and accepted is True
    inf.close()
