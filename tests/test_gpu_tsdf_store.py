"""GPU: what leaves the rolling TSDF window is kept and comes back (`ovn_tsdf_window_brick_flags / _page_out / _page_in`,
`tsdf_store.TsdfBrickStore`, `RollingTsdfVolume(store=)`, `RollingTsdfOdometry(store=)`).

The window is section 36's smallest hard shape, 72 x 24 x 16 at base (40, 8, 8) and at BASE_NEG: nx is no multiple of 64 and the seam
lies inside the volume on every axis.  Its content is the fused case of tests/_tsdf_window_ref.py, fused by the GPU.  The yardstick of
the paging is the NumPy model of tests/_tsdf_store_ref.py run side by side ON THE GPU'S OWN BITS, so nothing about the arithmetic of
fusion enters: every sample of the window and every stored brick, bit for bit, after every step.  The yardstick of the feature is the
dense volume: a window that went away and came back holds what it held, the mesh of window and store is the dense volume's mesh with no
triangle twice, and a drive out and back with known poses leaves the window with the bits of the fixed volume fused with the same
scans."""
import json

import numpy as np
import pytest
import torch

import _odometry_ref as OD
import _render_ref as R
import _tsdf_ref as T
import _tsdf_store_ref as SR
import _tsdf_window_ref as WR

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

SHAPE = WR.SHAPE
BASES = [WR.BASE, WR.BASE_NEG]
SEAM = tuple(b + n - b % n for b, n in zip(WR.BASE, SHAPE))
GUARD = 4096
MOVES = [(8, 0, 0), (-16, 8, 0), (80, 0, 0)]
FOV = dict(fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)


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


def _add(base, step):
    return tuple(int(b + s) for b, s in zip(base, step))


def _case_volume(eng, base, store=None, voxel=None, anchor=None, **kw):
    """A RollingTsdfVolume of SHAPE at `base` on the fused case's lattice (or on `voxel`, `anchor`)."""
    from overlapnet_amd import tsdf
    voxel = T.VOXEL if voxel is None else voxel
    vol = tsdf.RollingTsdfVolume(eng, tuple(n * voxel for n in SHAPE), voxel, trunc=T.TRUNC, max_weight=T.MAX_WEIGHT,
                                 anchor=WR.anchor_for(base) if anchor is None else anchor, store=store, **kw)
    assert vol.shape == SHAPE
    vol.base = tuple(base)
    return vol


def _fuse(vol, c, scans):
    vol.integrate(c["ranges"][scans], c["poses"][scans], **FOV)


def _host(vol):
    return vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()


def _flag_reference(t, w, lo, hi):
    """The NumPy reduction of a read-back window over the brick box lo .. hi: (hz,hy,hx) uint8."""
    out = np.zeros((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0]), np.uint8)
    for z in range(lo[2], hi[2]):
        for y in range(lo[1], hi[1]):
            for x in range(lo[0], hi[0]):
                ix = SR._brick_index((x, y, z), t.shape)
                out[z - lo[2], y - lo[1], x - lo[0]] = SR.brick_differs(t[ix], w[ix])
    return out


# ---- flags ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES, ids=["positive", "negative"])
def test_flags_are_the_reduction_of_the_window_bit_patterns_included(eng, base):
    from overlapnet_amd import tsdf
    from overlapnet_amd import tsdf_store as S
    c = T.fused_case(WR.CASE)
    vol = _case_volume(eng, base)
    _fuse(vol, c, slice(None))
    whole = S.brick_box(base, _add(base, SHAPE))
    # the fused case leaves no brick of this window untouched: six are cleared by hand, in the slabs the moves below make leave
    cleared = [(0, 0, 0), (8, 2, 1), (4, 1, 0), (7, 0, 1), (3, 2, 1), (8, 0, 0)]                  # brick offsets (x, y, z) from the base
    index = lambda off: SR._brick_index(tuple(o + l for o, l in zip(off, whole[0])), vol.tsdf.shape)
    for off in cleared:
        ix = index(off)
        vol.tsdf[int(ix[0][0, 0, 0]):int(ix[0][7, 0, 0]) + 1, int(ix[1][0, 0, 0]):int(ix[1][0, 7, 0]) + 1,
                 int(ix[2][0, 0, 0]):int(ix[2][0, 0, 7]) + 1] = 1.0
        vol.weight[int(ix[0][0, 0, 0]):int(ix[0][7, 0, 0]) + 1, int(ix[1][0, 0, 0]):int(ix[1][0, 7, 0]) + 1,
                   int(ix[2][0, 0, 0]):int(ix[2][0, 0, 7]) + 1] = 0.0
    t, w = _host(vol)
    before = _flag_reference(t, w, *whole)
    assert before.sum() == before.size - len(cleared) and all(before[z, y, x] == 0 for x, y, z in cleared)
    # two samples only their bits give away, each alone in a brick that is otherwise fresh
    planted = []
    for (x, y, z), (tv, wv) in zip(cleared[:2], ((0.5, 0.0), (1.0, -0.0))):
        ix = index((x, y, z))
        sz, sy, sx = int(ix[0][5, 0, 0]), int(ix[1][0, 2, 0]), int(ix[2][0, 0, 7])
        vol.tsdf[sz, sy, sx], vol.weight[sz, sy, sx] = tv, wv
        planted.append((z, y, x))
    t, w = _host(vol)
    assert w[w == 0].size and np.signbit(w).sum() == 1
    boxes = [whole] + [S.brick_box(lo, hi) for step in MOVES for lo, hi in tsdf.leaving_boxes(base, _add(base, step), SHAPE)]
    assert len(boxes) == 1 + 1 + 2 + 1
    for lo, hi in boxes:
        want = _flag_reference(t, w, lo, hi)
        flat = torch.full((want.size + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        got = S.window_brick_flags(eng, vol.tsdf, vol.weight, base, lo, hi, out=flat[GUARD:GUARD + want.size])
        assert got.data_ptr() == flat.data_ptr() + GUARD
        host = flat.cpu().numpy()
        print("flags %s .. %s at base %s: %d of %d bricks hold something" % (lo, hi, base, want.sum(), want.size))
        assert np.array_equal(host[GUARD:GUARD + want.size].reshape(want.shape), want)
        assert (host[:GUARD] == 0xAB).all() and (host[-GUARD:] == 0xAB).all()
        fresh = S.window_brick_flags(eng, vol.tsdf, vol.weight, base, lo, hi)
        assert tuple(fresh.shape) == want.shape and np.array_equal(fresh.cpu().numpy(), want)
    after = _flag_reference(t, w, *whole)
    for z, y, x in planted:
        assert before[z, y, x] == 0 and after[z, y, x] == 1
    assert after.sum() == before.sum() + 2


# ---- paging against the model --------------------------------------------------------------------------------------------------------
def _guarded_pool(store, slots=96, pattern=-7.5):
    """Gives the store a pool of `slots` slots inside a flat buffer with GUARD words of `pattern` on either side -> the buffer."""
    flat = torch.full((slots * 1024 + 2 * GUARD,), pattern, dtype=torch.float32, device="cuda")
    store._pool = flat[GUARD:GUARD + slots * 1024]
    return flat


def _compare(vol, model, what):
    t, w = _host(vol)
    assert vol.base == model.base, what
    assert t.size == 27648 and np.array_equal(_bits(t), _bits(model.tsdf)) and np.array_equal(_bits(w), _bits(model.weight)), what
    assert vol.store.bricks() == sorted(model.store) and len(vol.store) == len(model.store), what
    for k in vol.store.bricks():
        bt, bw = vol.store.get(k)
        assert np.array_equal(_bits(bt), _bits(model.store[k][0])) and np.array_equal(_bits(bw), _bits(model.store[k][1])), (what, k)


@pytest.mark.parametrize("base", BASES, ids=["positive", "negative"])
def test_paging_follows_the_model_on_every_sample_and_every_brick(eng, base):
    c = T.fused_case(WR.CASE)
    vol = _case_volume(eng, base, store=True)
    flat = _guarded_pool(vol.store)
    pool = vol.store._pool
    model = SR.Model(SHAPE, base)

    def fuse(scans, what):
        _fuse(vol, c, scans)
        model.tsdf, model.weight = _host(vol)                  # the model works on the GPU's own bits
        _compare(vol, model, what)

    def move(step, what):
        new = _add(vol.base, step)
        assert vol.follow(SR.position_for(vol, new)) and vol.base == new
        model.move(new)
        _compare(vol, model, what)
        print("%s: base %s, %d bricks stored (%d bytes)" % (what, vol.base, len(vol.store), vol.store.bytes))

    n = c["ranges"].shape[0]
    fuse(slice(0, n - 1), "fuse")
    held = []
    move((8, 0, 0), "+8 x")
    held.append(len(vol.store))
    fuse(slice(n - 1, n), "fuse one more scan")
    move((-16, 8, 0), "(-16, +8, 0)")
    held.append(len(vol.store))
    move((80, 0, 0), "+80 x: a whole window and more")
    held.append(len(vol.store))
    assert min(held) > 0
    move((-32, 0, 0), "back, first move")
    move((-40, -8, 0), "back, second move")
    assert vol.base == tuple(base) and vol.n_shifts == 5 and vol.pieces == []
    assert vol.store._pool is pool, "the guarded pool was replaced"
    host = flat.cpu().numpy()
    assert (host[:GUARD] == -7.5).all() and (host[-GUARD:] == -7.5).all()
    assert (host[GUARD + vol.store._top * 1024:-GUARD] == -7.5).all()       # no slot beyond those handed out was written


# ---- there and back ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", BASES, ids=["positive", "negative"])
def test_there_and_back_is_the_dense_volume(eng, base):
    c = T.fused_case(WR.CASE)
    away = _add(base, (SHAPE[0], 0, 0))                                     # a whole window along x
    differing = {}
    for store in (True, None):
        vol = _case_volume(eng, base, store=store)
        _fuse(vol, c, slice(None))
        t0, w0 = _host(vol)
        assert (w0 > 0).sum() > 1000
        assert vol.follow(SR.position_for(vol, away)) and vol.base == away
        t1, w1 = _host(vol)
        assert (_bits(t1) == SR.ONE_BITS).all() and (_bits(w1) == 0).all()  # nothing of the scene is out there
        assert vol.follow(SR.position_for(vol, base)) and vol.base == tuple(base)
        t2, w2 = _host(vol)
        differing[store] = int(((_bits(t2) != _bits(t0)) | (_bits(w2) != _bits(w0))).sum())
        if store:
            assert len(vol.store) == 0                                      # one home per brick: all of it is back in the window
        else:
            assert (_bits(t2) == SR.ONE_BITS).all() and (_bits(w2) == 0).all()
    print("there and back at base %s: %d of %d samples differ with a store, %d without" % (base, differing[True], t0.size, differing[None]))
    assert differing[True] == 0
    assert differing[None] > 0, "without a store the window forgets: the feature, not merely its names"


# ---- the mesh of window and store ----------------------------------------------------------------------------------------------------
ANCHOR, VOXEL = np.array([1.0, -2.0, 0.5]), 0.25
LONG = (3 * SHAPE[0], SHAPE[1], SHAPE[2])


def _key(tri):
    return sorted(np.ascontiguousarray(t).tobytes() for t in np.asarray(tri).reshape(-1, 3, 3))


def test_mesh_of_window_and_store_is_the_dense_mesh_with_no_triangle_twice(eng):
    base = WR.BASE
    # three windows along x; the plane leans so little along x that it crosses all three; one brick nobody has seen
    d, w = WR.plane_block(LONG, base, SEAM, normal=(0.03, -0.61, 0.70))
    vol = _case_volume(eng, base, store=True, voxel=VOXEL, anchor=ANCHOR)
    for i in range(3):
        at = _add(base, (i * SHAPE[0], 0, 0))
        if i:
            assert vol.follow(SR.position_for(vol, at))
        assert vol.base == at and bool((vol.weight == 0).all())
        cut = (slice(None), slice(None), slice(i * SHAPE[0], (i + 1) * SHAPE[0]))
        vol.tsdf.copy_(_dev(WR.to_ring(d[cut], at)))
        vol.weight.copy_(_dev(WR.to_ring(w[cut], at)))
    assert vol.follow(SR.position_for(vol, _add(base, (104, 0, 0))))        # back over the middle: window and store both hold bricks
    in_window = int((vol.weight > 0).sum())
    assert len(vol.store) > 0 and in_window > 0
    before = (_host(vol), vol.base, {k: vol.store.get(k) for k in vol.store.bricks()}, dict(vol.store._index), sorted(vol.store._free))
    tri = vol.triangles().cpu().numpy()
    mesh = vol.mesh()
    dense_shape = tuple(b + n + 8 for b, n in zip(base, LONG))
    dense, total = eng.tsdf_triangles(_dev(WR.in_dense(d, base, dense_shape)), _dev(WR.in_dense(w, base, dense_shape)), ANCHOR, VOXEL, 1.0)
    dense = dense.cpu().numpy()
    print("mesh sweep: %d triangles from window (%d seen samples) and %d stored bricks; the dense volume has %d"
          % (tri.shape[0], in_window, len(vol.store), total))
    assert total == dense.shape[0] > 1000 and tri.shape[0] == total
    xs = (dense[:, :, 0].min(axis=1) - ANCHOR[0]) / VOXEL
    for i in range(3):                                                      # the surface runs through all three windows
        assert ((xs >= base[0] + i * SHAPE[0]) & (xs < base[0] + (i + 1) * SHAPE[0])).sum() > 100, i
    got, want = _key(tri), _key(dense)
    # the plane passes through lattice points, where marching tetrahedra emits triangles of no area, several alike at one point: those
    # the dense mesh holds as often as the sweep; a triangle WITH an area belongs to one cell and must be there once
    e1, e2 = tri[:, 1].astype(np.float64) - tri[:, 0], tri[:, 2].astype(np.float64) - tri[:, 0]
    solid = _key(tri[np.abs(np.cross(e1, e2)).max(axis=1) > 0])
    print("mesh sweep: %d distinct triangles of %d, the dense mesh %d of %d; %d have an area, %d of those distinct"
          % (len(set(got)), len(got), len(set(want)), len(want), len(solid), len(set(solid))))
    assert got == want
    assert len(solid) > 20000 and len(set(solid)) == len(solid), "a triangle appears twice"
    assert mesh.n_triangles == total and _key(mesh.vertices) == got
    after = (_host(vol), vol.base, {k: vol.store.get(k) for k in vol.store.bricks()}, dict(vol.store._index), sorted(vol.store._free))
    assert after[1] == before[1] and after[3] == before[3] and after[4] == before[4]
    assert np.array_equal(_bits(after[0][0]), _bits(before[0][0])) and np.array_equal(_bits(after[0][1]), _bits(before[0][1]))
    assert sorted(after[2]) == sorted(before[2])
    for k in before[2]:
        assert np.array_equal(_bits(after[2][k][0]), _bits(before[2][k][0])) and np.array_equal(_bits(after[2][k][1]), _bits(before[2][k][1]))


# ---- the tracker ---------------------------------------------------------------------------------------------------------------------
NEAR = dict(extent=(17.6, 17.6, 8.0), max_range=6.0)                        # section 36's "near" run: the floor behind the sensor leaves
SENSOR = dict(proj_h=OD.HW[0], proj_w=OD.HW[1], fov_up=R.FOV_UP, fov_down=R.FOV_DOWN)


@pytest.fixture(scope="module")
def drive(eng):
    from overlapnet_amd.mesh import TriangleMesh
    world, rel = OD.drive()
    r = eng.render_scans(TriangleMesh(*R.scene(0)), world, OD.HW[0], OD.HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
    rng, vtx = r["range"].cpu().numpy(), r["vertex"].cpu().numpy()
    clouds = [np.ascontiguousarray(vtx[s][rng[s] > 0], np.float32) for s in range(OD.N_FRAMES)]
    lo, hi = OD.volume_box(world[0])
    return dict(clouds=clouds, lo=lo, hi=hi, rel=rel)


def _track(eng, drive, store):
    from overlapnet_amd import odometry
    odo = odometry.RollingTsdfOdometry(eng, NEAR["extent"], OD.VOXEL, trunc=OD.TRUNC, anchor=drive["lo"], shift=8, min_range=OD.MIN_RANGE,
                                       max_range=NEAR["max_range"], store=store, **SENSOR, **OD.ICP)
    moves = []
    for f, c in enumerate(drive["clouds"]):
        before = odo.volume.base
        odo.track(c)
        if f > 0 and odo.volume.base != before:
            moves.append((f, before, odo.volume.base))
    return odo, moves


def test_tracker_with_a_store_has_the_poses_of_the_one_without_and_the_fixed_mesh(eng, drive):
    from overlapnet_amd import odometry, tsdf
    plain, moves_plain = _track(eng, drive, None)
    kept, moves = _track(eng, drive, True)
    assert moves == moves_plain and len(moves) >= 2
    for a, b in zip(kept.results, plain.results):
        assert np.array_equal(a.pose.view(np.uint64), b.pose.view(np.uint64)) and a[1:] == b[1:]
    v = kept.volume
    assert len(v.store) > 0 and v.pieces == [] and len(plain.volume.pieces) >= 1
    # from the poses: no sample that left lay within reach of a scan fused after it left (the window never came back for it either)
    reach = (NEAR["max_range"] + OD.TRUNC + OD.VOXEL) / OD.VOXEL + 2.0
    poses = np.stack([r.pose for r in kept.results])
    for f, old, new in moves:
        for lo, hi in tsdf.leaving_boxes(old, new, v.shape):
            for g in range(f, OD.N_FRAMES):
                o = (poses[g, :3, 3] - v.anchor) / OD.VOXEL
                assert any((l - (o[a] + reach) > 0) or ((o[a] - reach) - (h - 1) > 0) for a, (l, h) in enumerate(zip(lo, hi))), \
                    "frame %d reaches the samples %s .. %s that left at frame %d" % (g, lo, hi, f)
    fixed = odometry.TsdfOdometry(eng, drive["lo"], drive["hi"], OD.VOXEL, trunc=OD.TRUNC, min_range=OD.MIN_RANGE,
                                  max_range=NEAR["max_range"], **SENSOR, **OD.ICP)
    for c in drive["clouds"]:
        fixed.track(c)
    dense = fixed.volume.triangles().cpu().numpy()
    mesh = v.mesh()
    print("near run with a store: %d moves, %d bricks stored, mesh %d triangles, the fixed volume's %d"
          % (len(moves), len(v.store), mesh.n_triangles, dense.shape[0]))
    assert mesh.n_triangles == dense.shape[0] > 1000 and _key(mesh.vertices) == _key(dense)
    with pytest.raises(ValueError, match="on_leave"):
        odometry.RollingTsdfOdometry(eng, NEAR["extent"], OD.VOXEL, trunc=OD.TRUNC, max_range=NEAR["max_range"], store=True,
                                     on_leave=lambda p: None, **SENSOR)
    with pytest.raises(ValueError, match="keep"):
        odometry.estimate_poses(eng, drive["clouds"][0], np.array([0, drive["clouds"][0].shape[0]], np.int64), keep=True)


def test_out_and_back_with_known_poses_is_the_fixed_volume(eng, drive):
    """Twelve scans fused at their true poses on the way out, the window brought back to frame 0, the twelve fused again on the way
    back: the window then holds the bits of the fixed volume fused with the same 24 scans in the same order -- provided every scan's
    reach lay in the window when it was fused, which is asserted from the poses first."""
    from overlapnet_amd import tsdf
    extent, max_range = (17.6, 17.6, 17.6), 6.0                             # 17.6 m on z too: the reach condition holds on every axis
    sensor = dict(SENSOR, max_range=max_range)
    rel = drive["rel"]
    vol = tsdf.RollingTsdfVolume(eng, extent, OD.VOXEL, trunc=OD.TRUNC, anchor=drive["lo"], shift=8, store=True)
    fixed = tsdf.TsdfVolume(eng, drive["lo"], drive["hi"], OD.VOXEL, trunc=OD.TRUNC)
    assert vol.shape == (88, 88, 88)
    paged = []
    page_in = vol.store.page_in
    vol.store.page_in = lambda *a, **k: paged.append(page_in(*a, **k)) or paged[-1]
    reach = (max_range + OD.TRUNC + OD.VOXEL) / OD.VOXEL
    order = list(range(OD.N_FRAMES)) + [None] + list(range(OD.N_FRAMES - 1, -1, -1))
    bases = []
    for s in order:
        if s is None:
            vol.follow(rel[0, :3, 3])                                        # the window comes back to frame 0 in one move
            continue
        vol.follow(rel[s, :3, 3])
        bases.append(vol.base)
        o = (rel[s, :3, 3] - vol.anchor) / OD.VOXEL
        for a in range(3):
            assert vol.base[a] <= o[a] - reach and o[a] + reach <= vol.base[a] + vol.shape[a] - 1, \
                "scan %d reaches past the window %s on axis %d: widen the window" % (s, vol.base, a)
        c = drive["clouds"][s]
        offs = np.array([0, c.shape[0]], np.int64)
        vol.integrate_scans(c, offs, rel[s:s + 1], **sensor)
        fixed.integrate_scans(c, offs, rel[s:s + 1], **sensor)
    assert vol.n_scans == fixed.n_scans == 24 and vol.n_shifts >= 4 and len(set(bases)) >= 3
    assert sum(paged) > 0, "nothing ever came back from the store"
    wt, ww = WR.to_block(vol.tsdf.cpu().numpy(), vol.base), WR.to_block(vol.weight.cpu().numpy(), vol.base)
    idx = [np.arange(n) + b for n, b in zip(vol.shape, vol.base)]
    inside = [(i >= 0) & (i < n) for i, n in zip(idx, (fixed.nx, fixed.ny, fixed.nz))]
    both = inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]
    assert both.any() and np.all(ww[~both] == 0) and np.all(wt[~both] == 1)          # outside the fixed box nothing was ever seen
    cut = tuple(slice(int(i[m].min()), int(i[m].max()) + 1) for i, m in zip(idx[::-1], inside[::-1]))
    ft, fw = fixed.tsdf.cpu().numpy()[cut], fixed.weight.cpu().numpy()[cut]
    sub = np.ix_(inside[2], inside[1], inside[0])
    differ = int(((_bits(wt[sub]) != _bits(ft)) | (_bits(ww[sub]) != _bits(fw))).sum())
    print("out and back: %d shifts over bases %s, %d bricks paged in, %d stored at the end; %d of %d shared samples differ (%d seen twice)"
          % (vol.n_shifts, sorted(set(bases)), sum(paged), len(vol.store), differ, ft.size, int((fw >= 2).sum())))
    assert (fw >= 2).sum() > 10000
    assert differ == 0


# ---- the tools -----------------------------------------------------------------------------------------------------------------------
def test_odometry_tool_keeps_saves_and_build_mesh_loads(drive, tmp_path, capsys):
    from overlapnet_amd.mesh import TriangleMesh
    from tools import build_mesh, odometry as tool
    scans = tmp_path / "scans"
    scans.mkdir()
    for s, c in enumerate(drive["clouds"]):
        c.tofile(str(scans / ("%06d.bin" % s)))
    cfg = tmp_path / "network.json"
    cfg.write_text(json.dumps({"model": {"inputShape": [OD.HW[0], OD.HW[1], 4]}}))
    out, ply, npz, again = (tmp_path / n for n in ("poses.txt", "site.ply", "map.npz", "again.ply"))
    common = ["--config", str(cfg), "--scans", str(scans), "--out", str(out)]
    tool.main(common + ["--max-range", "6", "--voxel", "0.2", "--window", "17.6", "--below", "3", "--above", "5", "--keep",
                        "--save-volume", str(npz), "--mesh", str(ply)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["volume"] == [88, 88, 40] and line["window_shifts"] >= 2 and line["stored_bricks"] > 0
    assert line["saved_bricks"] > line["stored_bricks"] and line["triangles"] > 1000
    build_mesh.main(["--load-volume", str(npz), "--out", str(again)])
    second = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert second["bricks"] == line["saved_bricks"] and second["triangles"] == line["triangles"]
    a, b = TriangleMesh.from_ply(str(ply)), TriangleMesh.from_ply(str(again))
    soup = lambda m: np.asarray(m.vertices, np.float32)[np.asarray(m.triangles).reshape(-1)]
    assert _key(soup(a)) == _key(soup(b))
    for extra, message in ((["--keep"], "--keep belongs to --window"), (["--window", "17.6", "--save-volume", str(npz)], "belongs to --keep")):
        with pytest.raises(SystemExit) as stop:
            tool.main(common + extra)
        assert stop.value.code == 2 and message in capsys.readouterr().err
    with pytest.raises(SystemExit) as stop:
        build_mesh.main(["--load-volume", str(npz), "--out", str(again), "--scans", str(scans)])
    assert stop.value.code == 2 and "--load-volume" in capsys.readouterr().err
