"""GPU: the rolling TSDF window (`ovn_tsdf_window_integrate / _raycast / _shift / _triangles`, `tsdf.RollingTsdfVolume`,
`odometry.RollingTsdfOdometry`).

A window sample is the lattice sample of a dense volume with origin = anchor, so the yardstick of every kernel is the dense kernel on
the same device: bit-equal, on every sample, pixel and triangle, with no exclusions.  The window is 72 x 24 x 16 at base (40, 8, 8): nx
is no multiple of 64 (a wave's run crosses the row end), the ring's seam lies inside a 64-lane run on x and inside the volume on y and
z.  A negative base has no dense volume to be compared with; there the NumPy statement on the block at index_offset = base is the
yardstick, under the rule of tests/test_gpu_tsdf.py (tests/test_tsdf_window_host.py holds the inputs to its cap on the CPU).  The
tracker follows the twelve-frame drive of tests/_odometry_ref.py in a 48 m x 48 m x 8 m window and must give the bits of the
fixed-volume tracker; its streamed mesh must be the fixed volume's mesh.  On that run nothing with a surface leaves the window (RUNS
says why), so the same two checks run once more with the sensor's range cut to 6 m, where a piece of the floor does."""
import ctypes as C

import numpy as np
import pytest
import torch

import _odometry_ref as OD
import _raycast_ref as RC
import _render_ref as R
import _tsdf_ref as T
import _tsdf_window_ref as WR

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

SHAPE, BASE, DENSE = WR.SHAPE, WR.BASE, WR.DENSE
CUT = (slice(BASE[2], BASE[2] + SHAPE[2]), slice(BASE[1], BASE[1] + SHAPE[1]), slice(BASE[0], BASE[0] + SHAPE[0]))
SEAM = tuple(b + n - b % n for b, n in zip(BASE, SHAPE))        # the lattice index in slot 0 of every axis: (72, 24, 16)
GUARD = 4096


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tbits(t):
    return t.contiguous().view(torch.int32)


def _fuse(eng, shape, anchor, ranges, poses, base=None, tsdf=None, weight=None):
    t0, w0 = T.fresh(shape)
    t, w = _dev(t0 if tsdf is None else tsdf), _dev(w0 if weight is None else weight)
    eng.tsdf_integrate(t, w, anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, _dev(ranges), poses, R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, base=base)
    return t.cpu().numpy(), w.cpu().numpy()


# ---- integrate -----------------------------------------------------------------------------------------------------------------------
def test_integrate_has_the_bits_of_the_dense_volume_that_contains_the_window(eng):
    c = T.fused_case(WR.CASE)
    anchor = WR.anchor_for(BASE)
    dt, dw = _fuse(eng, DENSE, anchor, c["ranges"], c["poses"])
    wt, ww = _fuse(eng, SHAPE, anchor, c["ranges"], c["poses"], base=BASE)
    bt, bw = WR.to_block(wt, BASE), WR.to_block(ww, BASE)
    print("window integrate: %d of %d samples updated, %d differ from the dense block" % ((bw > 0).sum(), bw.size, (_bits(bt) != _bits(dt[CUT])).sum()))
    assert (bw > 0).sum() > 1000 and (dw[CUT] > 0).sum() == (bw > 0).sum()
    assert np.array_equal(_bits(bt), _bits(dt[CUT])) and np.array_equal(_bits(bw), _bits(dw[CUT]))
    # on both sides of the seam of every axis
    for a in range(3):
        idx = np.arange(SHAPE[a]) + BASE[a]
        seen = (bw > 0).any(axis=tuple(x for x in range(3) if x != 2 - a))
        assert seen[idx < SEAM[a]].any() and seen[idx >= SEAM[a]].any(), a
    # two calls give the bits of one, on storage that is not fresh
    t2, w2 = _fuse(eng, SHAPE, anchor, c["ranges"][:2], c["poses"][:2], base=BASE)
    t2, w2 = _fuse(eng, SHAPE, anchor, c["ranges"][2:], c["poses"][2:], base=BASE, tsdf=t2, weight=w2)
    assert np.array_equal(_bits(t2), _bits(wt)) and np.array_equal(_bits(w2), _bits(ww))


def test_integrate_at_a_negative_base_matches_the_statement(eng):
    base = WR.BASE_NEG
    c = T.fused_case(WR.CASE)
    anchor = WR.anchor_for(base)
    t0, w0 = T.fresh(SHAPE)
    kw = dict(index_offset=base)
    ref = T.integrate(t0, w0, anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"], c["poses"], **kw)
    f64 = T.integrate(t0, w0, anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"], c["poses"], dtype=np.float64, ambiguous=True, **kw)
    wt, ww = _fuse(eng, SHAPE, anchor, c["ranges"], c["poses"], base=base)
    t, w = WR.to_block(wt, base), WR.to_block(ww, base)
    touched, amb = f64["updated"].any(axis=0), f64["ambiguous"]
    share = (amb & touched).sum() / max(int(touched.sum()), 1)
    differ = _bits(t) != _bits(ref["tsdf"])
    print("negative base: %d samples, %d updated, ambiguous share %.4f, %d differ from the statement (%d outside the ambiguous ones)"
          % (t.size, touched.sum(), share, differ.sum(), differ[~amb].sum()))
    assert share <= 0.05 and touched.sum() > 1000
    assert np.array_equal(_bits(t)[~amb], _bits(ref["tsdf"])[~amb]) and np.array_equal(_bits(w)[~amb], _bits(ref["weight"])[~amb])


# ---- shift ---------------------------------------------------------------------------------------------------------------------------
def _guarded(values, pattern):
    """A (nz,ny,nx) view into a flat buffer with GUARD words of `pattern` on either side -> (view, whole buffer)."""
    flat = torch.full((values.size + 2 * GUARD,), pattern, dtype=torch.float32, device="cuda")
    view = flat[GUARD:GUARD + values.size].view(values.shape)
    view.copy_(_dev(values))
    return view, flat


def test_shift_clears_the_slots_that_change_hands_and_nothing_else(eng):
    g = np.random.default_rng(17)
    nz, ny, nx = SHAPE[::-1]
    t = g.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    w = g.integers(1, 9, (nz, ny, nx)).astype(np.float32)
    dt, ft = _guarded(t, 7.25)
    dw, fw = _guarded(w, -3.5)
    base = BASE
    for step in ((8, 0, 0), (-16, 8, 0), (80, 0, 0)):
        new = tuple(b + s for b, s in zip(base, step))
        t, w, fresh = WR.shift(t, w, base, new)
        eng.tsdf_window_shift(dt, dw, base, new)
        print("shift %s: %d of %d slots change hands" % (step, fresh.sum(), fresh.size))
        assert 0 < fresh.sum() and (fresh.all() if step[0] >= nx else not fresh.all())
        assert np.array_equal(_bits(dt.cpu().numpy()), _bits(t)) and np.array_equal(_bits(dw.cpu().numpy()), _bits(w))
        for flat, pattern in ((ft, 7.25), (fw, -3.5)):
            assert bool((flat[:GUARD] == pattern).all()) and bool((flat[-GUARD:] == pattern).all())
        base = new
    before = dt.clone()
    eng.tsdf_window_shift(dt, dw, base, base)                       # no move: nothing is launched, nothing changes
    assert torch.equal(_tbits(dt), _tbits(before))


# ---- ray cast ------------------------------------------------------------------------------------------------------------------------
ANCHOR, VOXEL = np.array([1.0, -2.0, 0.5]), 0.25
HW = (16, 90)


def _plane_window():
    """The oblique plane through the seam's corner, in the window (ring storage) and in the dense volume that has seen nothing else."""
    d, w = WR.plane_block(SHAPE, BASE, SEAM)
    return WR.to_ring(d, BASE), WR.to_ring(w, BASE), WR.in_dense(d, BASE), WR.in_dense(w, BASE)


def _seam_poses():
    """Three sensors on the plane's positive side within a few voxels of the seam's corner, each looking at it."""
    nrm = np.array([0.37, -0.61, 0.70]) / np.linalg.norm([0.37, -0.61, 0.70])
    corner = ANCHOR + np.asarray(SEAM) * VOXEL
    eyes = [corner + (5.0 * nrm + np.array(off)) * VOXEL for off in ((0.3, 0.2, 0.1), (3.0, 2.5, 0.4), (-2.2, 1.1, 0.9))]
    return np.stack([RC.look_at(e, corner + np.array([0.11, 0.07, 0.0])) for e in eyes])


def test_raycast_has_the_bits_of_the_dense_raycast(eng):
    rt, rw, dd, dw = (_dev(a) for a in _plane_window())
    poses = _seam_poses()
    march = dict(fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, min_range=0.3, max_range=12.0, step=VOXEL, min_weight=1.0)
    want = ("range", "vertex", "normal")
    for masked in (False, True):
        mask_w = eng.tsdf_bricks(rw, 1.0) if masked else None
        mask_d = eng.tsdf_bricks(dw, 1.0) if masked else None
        win = eng.tsdf_raycast(rt, rw, ANCHOR, VOXEL, poses, HW[0], HW[1], bricks=mask_w, want=want, stacked_flags=(True, True), base=BASE, **march)
        den = eng.tsdf_raycast(dd, dw, ANCHOR, VOXEL, poses, HW[0], HW[1], bricks=mask_d, want=want, stacked_flags=(True, True), **march)
        for k in want + ("stacked",):
            assert torch.equal(_tbits(win[k]), _tbits(den[k])), (k, masked)
        if masked:
            assert int(mask_w.sum()) < mask_w.numel() and int(mask_w.sum()) == int(mask_d.sum())     # the unseen brick; the ring permutes bricks
    rng, vtx = win["range"].cpu().numpy(), win["vertex"].cpu().numpy().astype(np.float64)
    hit = rng > 0
    # where the hits lie on the lattice: cells that straddle the seam of every axis, and the rest of the image looks out of the window
    cells = []
    for s in range(poses.shape[0]):
        p = vtx[s][hit[s]][:, :3] @ poses[s, :3, :3].T + poses[s, :3, 3]
        cells.append(np.floor((p - ANCHOR) / VOXEL).astype(np.int64))
    cells = np.concatenate(cells)
    print("window raycast: %d of %d pixels hit, cells x %d..%d y %d..%d z %d..%d" % ((hit.sum(), hit.size) + tuple(
        v for a in range(3) for v in (cells[:, a].min(), cells[:, a].max()))))
    assert hit.sum() > 200 and (~hit).sum() > 200
    for a in range(3):
        assert (cells[:, a] == SEAM[a] - 1).any() and (cells[:, a] < SEAM[a] - 1).any() and (cells[:, a] >= SEAM[a]).any(), a
    # a sample outside the window is invalid whatever the storage holds: a window seen everywhere still ends at its faces
    full = eng.tsdf_raycast(rt, torch.ones_like(rw), ANCHOR, VOXEL, poses, HW[0], HW[1], want=("range",), base=BASE, **march)["range"]
    every = eng.tsdf_raycast(dd, _dev(WR.in_dense(np.ones(SHAPE[::-1], np.float32), BASE)), ANCHOR, VOXEL, poses, HW[0], HW[1],
                             want=("range",), **march)["range"]
    assert torch.equal(_tbits(full), _tbits(every)) and bool((full < 0).any())


# ---- triangles -----------------------------------------------------------------------------------------------------------------------
def _dense_triangles(eng, d_block, w_block, lo, hi):
    """ovn_tsdf_triangles of the dense volume with origin = anchor that has seen the samples of the cells lo .. hi (exclusive) only."""
    cut = tuple(slice(l - b, h - b + 1) for l, h, b in zip(lo[::-1], hi[::-1], BASE[::-1]))
    seen = np.zeros_like(w_block)
    seen[cut] = w_block[cut]
    tri, total = eng.tsdf_triangles(_dev(WR.in_dense(d_block, BASE)), _dev(WR.in_dense(seen, BASE)), ANCHOR, VOXEL, 1.0)
    return (tri.cpu().numpy() if total else np.zeros((0, 3, 3), np.float32)), total


def test_triangles_of_a_box_and_of_the_leaving_boxes_have_the_dense_bits(eng):
    from overlapnet_amd import _lib, tsdf
    from overlapnet_amd.engine import _ptr
    d, w = WR.plane_block(SHAPE, BASE, SEAM)
    rt, rw = _dev(WR.to_ring(d, BASE)), _dev(WR.to_ring(w, BASE))
    top = tuple(b + n - 1 for b, n in zip(BASE, SHAPE))
    new = tuple(b + 8 for b in BASE)                                  # a diagonal shift
    leaving = tsdf.leaving_boxes(BASE, new, tuple(n - 1 for n in SHAPE))
    assert len(leaving) == 3
    boxes = [((66, 20, 12), (78, 28, 20)), (BASE, top)] + leaving
    counts = []
    for lo, hi in boxes:
        got, total = eng.tsdf_triangles(rt, rw, ANCHOR, VOXEL, 1.0, base=BASE, box=(lo, hi))
        want, n = _dense_triangles(eng, d, w, lo, hi)
        counts.append(total)
        assert total == n > 0, (lo, hi)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (lo, hi)
    print("window triangles per box: %s" % counts)
    # the three leaving boxes are the whole window's cells that the shifted window does not hold
    stay, _ = eng.tsdf_triangles(rt, rw, ANCHOR, VOXEL, 1.0, base=BASE, box=(new, top))
    assert counts[1] == sum(counts[2:]) + int(stay.shape[0])
    # capacity and guard, as for ovn_tsdf_triangles: the first `cap` triangles, the total, and nothing beyond
    lo, hi = boxes[0]
    full, total = eng.tsdf_triangles(rt, rw, ANCHOR, VOXEL, 1.0, base=BASE, box=(lo, hi))
    cap = total // 2
    buf = torch.full((cap + 8, 3, 3), 5.5, dtype=torch.float32, device="cuda")
    part, n = eng.tsdf_triangles(rt, rw, ANCHOR, VOXEL, 1.0, capacity=cap, out=buf, base=BASE, box=(lo, hi))
    assert n == total and part.shape[0] == cap and torch.equal(_tbits(part), _tbits(full[:cap])) and bool((buf[cap:] == 5.5).all())
    assert eng.tsdf_triangles(rt, rw, ANCHOR, VOXEL, 1.0, capacity=0, base=BASE, box=(lo, hi)) == (None, total)
    assert eng.tsdf_triangles(rt, rw, ANCHOR, VOXEL, 1.0, base=BASE, box=((50, 10, 10), (50, 12, 12))) == (None, 0)     # an empty box
    # the library's own refusals leave the count word alone
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    i3 = lambda v: (C.c_int32 * 3)(*v)
    org = (C.c_double * 3)(*ANCHOR)
    nx, ny, nz = SHAPE
    for dims, base, lo, hi in (((70, ny, nz), BASE, lo, hi), ((nx, ny, 8), BASE, lo, hi), ((nx, ny, nz), (44, 8, 8), lo, hi),
                               ((nx, ny, nz), ((1 << 20) - 64, 8, 8), lo, hi), ((nx, ny, nz), BASE, (39, 8, 8), hi),
                               ((nx, ny, nz), BASE, lo, (112, 28, 20)), ((nx, ny, nz), BASE, hi, lo)):
        rc = eng.lib.ovn_tsdf_window_triangles(eng._h, None, _ptr(rt), _ptr(rw), dims[0], dims[1], dims[2], org, i3(base), VOXEL, 1.0,
                                               i3(lo), i3(hi), None, 0, _ptr(count))
        assert rc == 1, (dims, base, lo, hi)
    assert eng.lib.ovn_tsdf_window_shift(eng._h, None, _ptr(rt), _ptr(rw), nx, ny, nz, i3(BASE), i3((44, 8, 8))) == 1
    assert int(count.item()) == -7
    with pytest.raises(_lib.OvnError):
        eng.tsdf_integrate(rt, rw, ANCHOR, VOXEL, 1.0, 64.0, torch.zeros((1, 4, 8), device="cuda"), np.eye(4)[None], base=(40, 8, 12))


# ---- the tracker that follows ------------------------------------------------------------------------------------------------------------
SENSOR = dict(proj_h=OD.HW[0], proj_w=OD.HW[1], fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)
SHIFT = 8
# name -> (window in metres, max_range).  "drive": the sensor as it is.  A window that holds all a scan reaches from anywhere within
# `shift` voxels of its centre loses a surface only after some 2 * shift voxels of travel beyond the sensor's range, which twelve frames
# of 0.5 m do not cover at 20 m: every piece of that run is empty.  "near" tracks the same clouds with the range cut to 6 m, in the
# smallest window the tracker accepts for it (8.8 m >= 6 + 0.8 + 0.2 + 1.6), so that the floor behind the sensor leaves the window.
RUNS = {"drive": ((48.0, 48.0, 8.0), R.MAX_RANGE), "near": ((17.6, 17.6, 8.0), 6.0)}


@pytest.fixture(scope="module")
def drive(eng):
    from overlapnet_amd.mesh import TriangleMesh
    world, rel = OD.drive()
    r = eng.render_scans(TriangleMesh(*R.scene(0)), world, OD.HW[0], OD.HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
    rng, vtx = r["range"].cpu().numpy(), r["vertex"].cpu().numpy()
    clouds = [np.ascontiguousarray(vtx[s][rng[s] > 0], np.float32) for s in range(OD.N_FRAMES)]
    lo, hi = OD.volume_box(world[0])
    return dict(clouds=clouds, lo=lo, hi=hi, rel=rel)


def _sensor(run):
    return dict(SENSOR, max_range=RUNS[run][1])


def _follow(eng, drive, run):
    """The drive in the window -> (tracker, results, [(frame, old base, new base)] of the moves after the first placement)."""
    from overlapnet_amd import odometry
    odo = odometry.RollingTsdfOdometry(eng, RUNS[run][0], OD.VOXEL, trunc=OD.TRUNC, anchor=drive["lo"], shift=SHIFT, min_range=OD.MIN_RANGE,
                                       **_sensor(run), **OD.ICP)
    results, moves = [], []
    for f, c in enumerate(drive["clouds"]):
        before = odo.volume.base
        results.append(odo.track(c))
        if f > 0 and odo.volume.base != before:
            moves.append((f, before, odo.volume.base))
    return odo, results, moves


@pytest.fixture(scope="module", params=sorted(RUNS))
def tracked(request, eng, drive):
    from overlapnet_amd import odometry
    run = request.param
    fixed = odometry.TsdfOdometry(eng, drive["lo"], drive["hi"], OD.VOXEL, trunc=OD.TRUNC, min_range=OD.MIN_RANGE, **_sensor(run), **OD.ICP)
    fixed_results = [fixed.track(c) for c in drive["clouds"]]
    odo, results, moves = _follow(eng, drive, run)
    return dict(run=run, fixed=fixed, fixed_results=fixed_results, odo=odo, results=results, moves=moves)


def test_following_tracker_gives_the_bits_of_the_fixed_volume(tracked):
    odo, moves, run = tracked["odo"], tracked["moves"], tracked["run"]
    print("%s: window %s at base %s after %d moves: %s; sources %s" % (run, odo.volume.shape, odo.volume.base, len(moves), moves,
                                                                       [r.source for r in tracked["results"]]))
    assert odo.volume.shape == {"drive": (240, 240, 40), "near": (88, 88, 40)}[run]
    assert len(moves) >= 2, "the window must move at least twice on this drive"
    for a, b in zip(tracked["results"], tracked["fixed_results"]):
        assert np.array_equal(a.pose.view(np.uint64), b.pose.view(np.uint64)) and a[1:] == b[1:]
    if run == "drive":
        assert [r.source for r in tracked["results"][1:]] == ["model"] * (OD.N_FRAMES - 1)
    # what the argument rests on: a window sample outside the fixed box was never seen, and every sample both hold has the same bits
    v, f = odo.volume, tracked["fixed"].volume
    wt, ww = WR.to_block(v.tsdf.cpu().numpy(), v.base), WR.to_block(v.weight.cpu().numpy(), v.base)
    idx = [np.arange(n) + b for n, b in zip(v.shape, v.base)]
    inside = [(i >= 0) & (i < n) for i, n in zip(idx, (f.nx, f.ny, f.nz))]
    both = inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]
    assert both.any() and not both.all() and np.all(ww[~both] == 0) and np.all(wt[~both] == 1)
    cut = tuple(slice(int(i[m].min()), int(i[m].max()) + 1) for i, m in zip(idx[::-1], inside[::-1]))
    ft, fw = f.tsdf.cpu().numpy()[cut], f.weight.cpu().numpy()[cut]
    sub = np.ix_(inside[2], inside[1], inside[0])
    seen = ww[sub] > 0                                   # the window forgot what left it; what it holds is the fixed volume's
    assert seen.sum() > 10000 and np.array_equal(_bits(wt[sub][seen]), _bits(ft[seen])) and np.array_equal(_bits(ww[sub][seen]), _bits(fw[seen]))


def test_streamed_mesh_is_the_fixed_volume_s_mesh(tracked):
    from overlapnet_amd import tsdf
    odo, moves = tracked["odo"], tracked["moves"]
    v = odo.volume
    # on the host, from the poses: no sample of an emitted cell lay within reach of a scan fused after the cell was emitted.  A scan
    # changes the samples within max_range + trunc + voxel of its sensor along every axis, plus one index (ovn_tsdf_integrate)
    reach = (RUNS[tracked["run"]][1] + OD.TRUNC + OD.VOXEL) / OD.VOXEL + 2.0
    poses = np.stack([r.pose for r in tracked["results"]])
    for f, old, new in moves:
        for lo, hi in tsdf.leaving_boxes(old, new, tuple(n - 1 for n in v.shape)):
            for g in range(f, OD.N_FRAMES):
                o = (poses[g, :3, 3] - v.anchor) / OD.VOXEL
                apart = [(l - (o[a] + reach) > 0) or ((o[a] - reach) - h > 0) for a, (l, h) in enumerate(zip(lo, hi))]      # samples lo .. hi
                assert any(apart), "frame %d reaches the cells %s .. %s that left at frame %d: widen the window" % (g, lo, hi, f)
    pieces = list(v.pieces) + [v.triangles().cpu().numpy()]
    streamed = np.concatenate(pieces)
    dense = tracked["fixed"].volume.triangles().cpu().numpy()
    print("%s: streamed mesh: %d triangles in %d pieces (%s), the fixed volume's mesh has %d"
          % (tracked["run"], streamed.shape[0], len(pieces), [p.shape[0] for p in pieces], dense.shape[0]))
    key = lambda tri: sorted(np.ascontiguousarray(t).tobytes() for t in tri)
    if tracked["run"] == "near":
        assert len(v.pieces) >= 1 and sum(p.shape[0] for p in v.pieces) > 100, "nothing left the window: the run streams no mesh"
    assert streamed.shape[0] == dense.shape[0] > 1000
    assert key(streamed) == key(dense)
    mesh = v.mesh()
    assert mesh.n_triangles == dense.shape[0] and np.array_equal(_bits(mesh.vertices.reshape(-1, 3, 3)), _bits(streamed))


def test_two_runs_give_the_same_bits(eng, drive, tracked):
    odo, results, moves = _follow(eng, drive, tracked["run"])
    assert moves == tracked["moves"]
    for a, b in zip(results, tracked["results"]):
        assert np.array_equal(a.pose.view(np.uint64), b.pose.view(np.uint64)) and a[1:] == b[1:]
    assert torch.equal(_tbits(odo.volume.tsdf), _tbits(tracked["odo"].volume.tsdf))
    assert torch.equal(_tbits(odo.volume.weight), _tbits(tracked["odo"].volume.weight))
    assert len(odo.volume.pieces) == len(tracked["odo"].volume.pieces)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(odo.volume.pieces, tracked["odo"].volume.pieces))


def test_estimate_poses_in_a_window_runs_where_the_fixed_box_does_not_fit(eng, drive):
    """Two scans at a 0.02 m voxel: the fixed box, 40 m x 40 m x 20 m and more, is over 2^31 - 1 samples; the window is 42 m x 42 m x
    0.32 m, 70 million."""
    from overlapnet_amd import odometry
    clouds = drive["clouds"][:2]
    points = np.concatenate(clouds)
    offsets = np.array([0, clouds[0].shape[0], points.shape[0]], np.int64)
    kw = dict(voxel=0.02, min_range=OD.MIN_RANGE, **SENSOR, **OD.ICP)
    with pytest.raises(ValueError, match="2\\^31"):
        odometry.estimate_poses(eng, points, offsets, **kw)
    poses, results, vol = odometry.estimate_poses(eng, points, offsets, window=(42.0, 42.0, 0.32), **kw)
    assert poses.shape == (2, 4, 4) and np.array_equal(poses[0], np.eye(4)) and np.isfinite(poses).all()
    assert vol.shape == (2104, 2104, 16) and vol.n_scans >= 1 and results[0].source == "first"
    assert results[1].source in ("model", "frame", "prediction") and bool((vol.weight > 0).any())


def test_odometry_tool_tracks_in_a_window_and_writes_the_streamed_mesh(drive, tmp_path, capsys):
    import json
    from overlapnet_amd.mesh import TriangleMesh
    from tools import odometry as tool
    from tools.build_training_set import read_poses
    scans = tmp_path / "scans"
    scans.mkdir()
    for s, c in enumerate(drive["clouds"]):
        c.tofile(str(scans / ("%06d.bin" % s)))
    cfg = tmp_path / "network.json"
    cfg.write_text(json.dumps({"model": {"inputShape": [OD.HW[0], OD.HW[1], 4]}}))
    out, ply = tmp_path / "poses.txt", tmp_path / "site.ply"
    tool.main(["--config", str(cfg), "--scans", str(scans), "--max-range", str(R.MAX_RANGE), "--out", str(out), "--voxel", "0.2",
               "--window", "48", "--below", "3", "--above", "5", "--mesh", str(ply)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    poses = read_poses(str(out))
    assert poses.shape == (OD.N_FRAMES, 4, 4) and np.array_equal(poses[0], np.eye(4))
    assert line["mode"] == "frame_to_model" and line["volume"] == [240, 240, 40] and line["window_m"] == 48.0 and line["window_shifts"] >= 2
    assert line["sources"]["model"] == OD.N_FRAMES - 1
    dt, dr = OD.distances(poses, drive["rel"])
    print("tools/odometry.py --window 48: translation max %.4f m, rotation max %.4f deg, %d shifts" % (dt.max(), dr.max(), line["window_shifts"]))
    assert dt.max() < 0.05 and dr.max() < 0.5                   # the bounds tests/test_gpu_odometry.py sets for the tool on this drive
    assert TriangleMesh.from_ply(str(ply)).n_triangles == line["triangles"] > 1000
    with pytest.raises(SystemExit, match="max_range"):
        tool.main(["--config", str(cfg), "--scans", str(scans), "--max-range", str(R.MAX_RANGE), "--out", str(out), "--window", "30"])
