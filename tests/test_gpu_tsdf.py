"""GPU: `ovn_tsdf_integrate` and `ovn_tsdf_triangles` (csrc/tsdf.hip) against their NumPy statement
(tests/_tsdf_ref.py) bit for bit, their properties and refusals, and the closed loop scans + poses -> mesh -> virtual scans -> map.

Integration: the target is every sample.  A differing sample is tolerated only where the float64 reference marks it ambiguous (a pixel
coordinate within 1e-3 of an integer, |sdf| within 1e-5 m of the truncation, depth within 1e-5 of 0), and the share of those is
asserted <= 5 % so that the exclusion cannot hide a failure.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import _render_ref as R
import _tsdf_ref as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

OVN_ERR_ARG = 1
TRIG = {"svml": "numpy_avx512", "f64": "rounded"}


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fuse(eng, shape, origin, ranges, poses, tsdf=None, weight=None, max_weight=T.MAX_WEIGHT, trunc=T.TRUNC, max_range=R.MAX_RANGE):
    """One ovn_tsdf_integrate call on a fresh (or the given) volume -> (tsdf, weight) host arrays."""
    t0, w0 = T.fresh(shape)
    t = _dev(t0 if tsdf is None else tsdf)
    w = _dev(w0 if weight is None else weight)
    eng.tsdf_integrate(t, w, origin, T.VOXEL, trunc, max_weight, _dev(ranges), poses, R.FOV_UP, R.FOV_DOWN, max_range)
    return t.cpu().numpy(), w.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 4. integration against the float32 statement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,trig", [("33x17x9", "svml"), ("33x17x9", "f64"), ("70x5x3", "svml"), ("2x2x2", "svml"),
                                       ("2x2x2_16x90", "svml")])
def test_integration_matches_the_statement(eng, name, trig):
    c = T.fused_case(name, trig)
    ref, f64 = c["f32"], c["f64"]
    eng.set_projection_trig(TRIG[trig])
    try:
        # scan by scan, so that every scan's updated / skipped decision shows in the weight
        t, w = T.fresh(c["shape"])
        decided = np.zeros_like(ref["updated"])
        for s in range(5):
            t, w2 = _fuse(eng, c["shape"], c["origin"], c["ranges"][s:s + 1], c["poses"][s:s + 1], t, w)
            decided[s] = w2 != w
            w = w2
        t1, w1 = _fuse(eng, c["shape"], c["origin"], c["ranges"], c["poses"])
    finally:
        eng.set_projection_trig("numpy_avx512")
    assert np.array_equal(_bits(t1), _bits(t)) and np.array_equal(_bits(w1), _bits(w))       # five calls of one = one call of five
    touched = f64["updated"].any(axis=0)
    amb = f64["ambiguous"]
    share = (amb & touched).sum() / max(int(touched.sum()), 1)
    clear = ~amb
    differing = int((_bits(t) != _bits(ref["tsdf"])).sum())
    print("%s %s: %d samples, %d updated, ambiguous share %.4f, %d samples differ from the statement (%d outside the ambiguous ones)"
          % (name, trig, t.size, touched.sum(), share, differing, (_bits(t) != _bits(ref["tsdf"]))[clear].sum()))
    assert share <= 0.05
    assert touched.any()
    assert np.array_equal(decided[:, clear], ref["updated"][:, clear])
    assert np.array_equal(_bits(t)[clear], _bits(ref["tsdf"])[clear])
    assert np.array_equal(_bits(w)[clear], _bits(ref["weight"])[clear])


# ---- 5. properties ------------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one(eng):
    c = T.fused_case("33x17x9")
    t, w = _fuse(eng, c["shape"], c["origin"], c["ranges"][:2], c["poses"][:2])
    t, w = _fuse(eng, c["shape"], c["origin"], c["ranges"][2:], c["poses"][2:], t, w)
    t1, w1 = _fuse(eng, c["shape"], c["origin"], c["ranges"], c["poses"])
    assert np.array_equal(_bits(t), _bits(t1)) and np.array_equal(_bits(w), _bits(w1))
    assert (w1 > 0).any()


def test_scan_alone_equals_scan_among_blind_poses(eng):
    c = T.fused_case("33x17x9")
    alone = _fuse(eng, c["shape"], c["origin"], c["ranges"][1:2], c["poses"][1:2])
    far = c["poses"].copy()
    far[[0, 2, 3, 4], :3, 3] += np.array([[300.0, 0, 0], [0, -300.0, 0], [0, 0, 300.0], [-1e6, 1e6, 0]])
    among = _fuse(eng, c["shape"], c["origin"], c["ranges"], far)
    assert np.array_equal(_bits(alone[0]), _bits(among[0])) and np.array_equal(_bits(alone[1]), _bits(among[1]))
    assert (alone[1] > 0).any()
    # and four blind poses alone leave the volume fresh
    t, w = _fuse(eng, c["shape"], c["origin"], c["ranges"][[0, 2, 3, 4]], far[[0, 2, 3, 4]])
    assert np.all(t == 1) and np.all(w == 0)


def test_non_finite_pose_skips_only_its_scan(eng):
    c = T.fused_case("33x17x9")
    for entry, value in (((0, 3), np.nan), ((1, 1), np.inf), ((2, 3), 1e300)):
        bad = c["poses"].copy()
        bad[1][entry] = value
        got = _fuse(eng, c["shape"], c["origin"], c["ranges"], bad)
        rest = [0, 2, 3, 4]
        want = _fuse(eng, c["shape"], c["origin"], c["ranges"][rest], c["poses"][rest])
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1])), entry
        assert (want[1] > 0).any()


def test_weight_saturates(eng):
    c = T.fused_case("33x17x9")
    rng, poses = np.repeat(c["ranges"][:1], 5, 0), np.repeat(c["poses"][:1], 5, 0)
    t, w = _fuse(eng, c["shape"], c["origin"], rng, poses, max_weight=2.0)
    assert set(np.unique(w)) == {0.0, 2.0}
    t0, w0 = T.fresh(c["shape"])
    ref = T.integrate(t0, w0, c["origin"], T.VOXEL, T.TRUNC, 2.0, rng, poses)
    amb = c["f64"]["ambiguous"]
    assert np.array_equal(_bits(t)[~amb], _bits(ref["tsdf"])[~amb]) and np.array_equal(_bits(w)[~amb], _bits(ref["weight"])[~amb])


def test_samples_above_the_field_of_view_stay_fresh(eng):
    rng, poses = T.scans(16, 90)
    # 9 x 9 x 5 samples from 2 m ahead of sensor 0 and 3 m above it: every one is more than 30 degrees above the horizon, where
    # the top row (+3 degrees, the room's far wall) must not be consulted
    origin = poses[0, :3, 3] + poses[0, :3, :3] @ np.array([2.0, -0.8, 3.0])
    assert (rng[0, 0] > 0).mean() > 0.5                                # the top row does see something
    t, w = _fuse(eng, (9, 9, 5), origin, rng[:1], poses[:1])
    assert np.all(t == 1) and np.all(w == 0)
    # the same box at the sensor's own height is updated
    origin = poses[0, :3, 3] + poses[0, :3, :3] @ np.array([2.0, -0.8, -1.0])
    t, w = _fuse(eng, (9, 9, 5), origin, rng[:1], poses[:1])
    assert (w > 0).mean() > 0.5


def test_every_refusal_leaves_the_volume_untouched(eng):
    lib, h = eng.lib, eng._h
    nx, ny, nz = 6, 5, 4
    g = np.random.default_rng(3)
    t0 = g.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)
    w0 = g.integers(0, 5, (nz, ny, nx)).astype(np.float32)
    t, w = _dev(t0), _dev(w0)
    rng = _dev(np.full((2, 4, 8), 3.0, np.float32))
    poses = _dev(np.tile(np.eye(4), (2, 1, 1)))
    org = (C.c_double * 3)(-1.0, -1.0, -1.0)
    nan_org = (C.c_double * 3)(-1.0, float("nan"), -1.0)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    good = dict(t=t, w=w, nx=nx, ny=ny, nz=nz, org=org, voxel=0.5, trunc=1.0, mw=8.0, rng=rng, poses=poses, n=2, H=4, W=8, mr=20.0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ovn_tsdf_integrate(h, p(a["t"]), p(a["w"]), a["nx"], a["ny"], a["nz"], a["org"], a["voxel"], a["trunc"], a["mw"],
                                      p(a["rng"]), p(a["poses"]), a["n"], a["H"], a["W"], 3.0, -25.0, a["mr"], None)

    nan = float("nan")
    refusals = [dict(t=None), dict(w=None), dict(org=None), dict(org=nan_org), dict(rng=None), dict(poses=None), dict(nx=1), dict(ny=1),
                dict(nz=0), dict(nx=65536, ny=65536), dict(nx=2048, ny=2048, nz=512), dict(voxel=0.0), dict(voxel=-0.5), dict(voxel=nan),
                dict(trunc=0.0), dict(trunc=nan), dict(mw=0.0), dict(mw=nan), dict(mr=0.0), dict(mr=-1.0), dict(mr=nan), dict(H=0),
                dict(W=0), dict(n=-1)]
    for kw in refusals:
        assert call(**kw) == OVN_ERR_ARG, kw
        assert b"ovn_tsdf_integrate" in lib.ovn_last_error()
    assert lib.ovn_tsdf_integrate(None, p(t), p(w), nx, ny, nz, org, 0.5, 1.0, 8.0, p(rng), p(poses), 2, 4, 8, 3.0, -25.0, 20.0,
                                  None) == OVN_ERR_ARG
    assert call(n=0) == 0 and call(n=0, rng=None, poses=None) == 0           # a no-op
    torch.cuda.synchronize()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(t0)) and np.array_equal(_bits(w.cpu().numpy()), _bits(w0))
    # ovn_tsdf_triangles: its refusals leave the count word and the output alone
    count = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    out = torch.full((4, 3, 3), 9.0, device="cuda")

    def tri(**kw):
        a = dict(good, mw=1.0, out=out, cap=4, count=count)
        a.update(kw)
        return lib.ovn_tsdf_triangles(h, p(a["t"]), p(a["w"]), a["nx"], a["ny"], a["nz"], a["org"], a["voxel"], a["mw"], p(a["out"]),
                                      a["cap"], p(a["count"]), None)

    for kw in (dict(t=None), dict(w=None), dict(count=None), dict(org=None), dict(org=nan_org), dict(nx=1), dict(nx=65536, ny=65536),
               dict(voxel=0.0), dict(voxel=nan), dict(mw=nan), dict(cap=-1)):
        assert tri(**kw) == OVN_ERR_ARG, kw
        assert b"ovn_tsdf_triangles" in lib.ovn_last_error()
    torch.cuda.synchronize()
    assert int(count.item()) == -7 and bool((out == 9.0).all())
    assert call() == 0 and tri() == 0                                         # and the good call runs
    torch.cuda.synchronize()
    assert int(count.item()) >= 0
    with pytest.raises(Exception):
        eng.tsdf_integrate(t, w[:2], (0, 0, 0), 0.5, 1.0, 8.0, rng, np.tile(np.eye(4), (2, 1, 1)))
    with pytest.raises(Exception):
        eng.tsdf_integrate(t, w, (0, 0, 0), 0.5, 1.0, 8.0, rng, np.tile(np.eye(4), (3, 1, 1)))


# ---- 6. extraction against the NumPy reference -----------------------------------------------------------------------------------
def _patterns_volume():
    """Random signs and magnitudes, some corners exactly 0 or -0 (zero-area triangles), some unseen.  (Every one of the 254 patterns of a
    cell on its own: test_extraction_one_cell_every_sign_pattern.)"""
    g = np.random.default_rng(11)
    d = (g.uniform(0.05, 1.0, (7, 8, 9)) * g.choice([-1.0, 1.0], (7, 8, 9))).astype(np.float32)
    d[g.uniform(size=d.shape) < 0.03] = 0.0
    d[g.uniform(size=d.shape) < 0.01] = -0.0
    w = np.where(g.uniform(size=d.shape) < 0.05, 0.0, g.integers(1, 4, d.shape)).astype(np.float32)
    return d, w, np.array([0.3, -7.0, 100.0]), 0.37


def _volumes():
    out = {"sphere": T.sphere_volume()[:4], "plane": T.plane_volume()[:4], "strip65x3x3": T.strip_volume()[:4],
           "patterns": _patterns_volume()}
    return out


@pytest.mark.parametrize("name", ["sphere", "plane", "strip65x3x3", "patterns", "fused"])
def test_extraction_matches_the_reference(eng, name):
    if name == "fused":
        c = T.fused_case("33x17x9")
        d, w = _fuse(eng, c["shape"], c["origin"], c["ranges"], c["poses"])        # the GPU's own volume
        origin, voxel = c["origin"], T.VOXEL
    else:
        d, w, origin, voxel = _volumes()[name]
    for min_weight in ((1.0, 2.0) if name in ("patterns", "fused") else (1.0,)):
        ref = T.triangles(d, w, origin, voxel, min_weight)
        tri, total = eng.tsdf_triangles(_dev(d), _dev(w), origin, voxel, min_weight)
        print("%s min_weight %g: %d triangles" % (name, min_weight, total))
        assert total == ref.shape[0] and total > 0
        assert np.array_equal(_bits(tri.cpu().numpy()), _bits(ref))
    if name == "strip65x3x3":
        # live cells on both sides of every boundary between runs of 64 cells
        counts = np.zeros(256, int)
        cells = np.floor((ref.astype(np.float64).mean(axis=1) - origin) / voxel + 1e-6).astype(int)
        np.add.at(counts, (cells[:, 2] * 2 + cells[:, 1]) * 64 + cells[:, 0], 1)
        for b in (64, 128, 192):
            assert counts[b - 1] > 0 and counts[b] > 0


def test_extraction_one_cell_every_sign_pattern(eng):
    """The smallest volume, 2 x 2 x 2 (one cell, one workgroup with 127 idle lanes), under each of the 254 sign patterns and the two
    without a surface: count, order and vertices bit for bit."""
    origin, voxel = T.ONE_CELL_ORIGIN, T.ONE_CELL_VOXEL
    w = np.ones((2, 2, 2), np.float32)
    dw = _dev(w)
    seen = 0
    for pattern, inside, d in T.one_cell_volumes():
        ref = T.triangles(d, w, origin, voxel)
        tri, total = eng.tsdf_triangles(_dev(d), dw, origin, voxel)
        assert total == ref.shape[0] and 1 <= total <= 12, pattern
        assert np.array_equal(_bits(tri.cpu().numpy()), _bits(ref)), pattern
        seen += 1
    assert seen == 254
    for value in (1.0, -1.0):
        assert eng.tsdf_triangles(_dev(np.full((2, 2, 2), value, np.float32)), dw, origin, voxel)[1] == 0


def test_extraction_min_weight_kills_the_cells_around_a_corner(eng):
    d, w, origin, voxel = T.plane_volume()[:4]
    full = T.triangles(d, w, origin, voxel)
    d, w2, origin, voxel, gone = T.unseen_corner_volume()
    tri, total = eng.tsdf_triangles(_dev(d), _dev(w2), origin, voxel)
    tri = tri.cpu().numpy()
    cells = np.floor((full.astype(np.float64).mean(axis=1) - origin) / voxel + 1e-9).astype(int)
    keep = np.array([tuple(c) not in gone for c in cells])
    assert 0 < keep.sum() < full.shape[0] and total == keep.sum()
    assert np.array_equal(_bits(tri), _bits(full[keep]))                      # exactly the eight cells around the sample are gone
    tri, total = eng.tsdf_triangles(_dev(d), _dev(w2), origin, voxel, min_weight=0.5)
    assert total == full.shape[0] and np.array_equal(_bits(tri.cpu().numpy()), _bits(full))


def test_extraction_capacity_and_determinism(eng):
    d, w, origin, voxel = T.sphere_volume()[:4]
    ref = T.triangles(d, w, origin, voxel)
    T_ = ref.shape[0]
    dd, dw = _dev(d), _dev(w)
    none, total = eng.tsdf_triangles(dd, dw, origin, voxel, capacity=0)           # counting only
    assert none is None and total == T_
    guard = 12345.0
    for cap in (T_, T_ - 1, 1, T_ + 5):
        buf = torch.full((T_ + 6, 3, 3), guard, device="cuda")
        tri, total = eng.tsdf_triangles(dd, dw, origin, voxel, capacity=cap, out=buf)
        n = min(cap, T_)
        assert total == T_ and tri.shape[0] == n
        assert np.array_equal(_bits(tri.cpu().numpy()), _bits(ref[:n]))
        assert bool((buf[n:] == guard).all())                                       # nothing beyond, the guard words intact
    # the C ABI with a buffer and capacity 0 (the wrapper would pass no buffer): the count, and not a word written
    buf = torch.full((4, 3, 3), guard, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    org = (C.c_double * 3)(*[float(x) for x in origin])
    rc = eng.lib.ovn_tsdf_triangles(eng._h, C.c_void_p(dd.data_ptr()), C.c_void_p(dw.data_ptr()), 16, 16, 16, org, float(voxel), 1.0,
                                    C.c_void_p(buf.data_ptr()), 0, C.c_void_p(count.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count.item()) == T_ and bool((buf == guard).all())
    a, _ = eng.tsdf_triangles(dd, dw, origin, voxel)
    b, _ = eng.tsdf_triangles(dd, dw, origin, voxel)
    assert torch.equal(a, b) and a.shape[0] == T_
    # a volume with no surface: T = 0, and TsdfVolume.mesh says so
    from overlapnet_amd import tsdf
    from overlapnet_amd._lib import OvnError
    vol = tsdf.TsdfVolume(eng, (0, 0, 0), (1, 1, 1), 0.25)
    assert (vol.nx, vol.ny, vol.nz) == (5, 5, 5)
    assert eng.tsdf_triangles(vol.tsdf, vol.weight, vol.origin, vol.voxel)[1] == 0
    with pytest.raises(OvnError, match="no surface"):
        vol.mesh()


# ---- 7. the closed loop ------------------------------------------------------------------------------------------------------------
BUILD_HW, EVAL_HW = (32, 360), (16, 90)


@pytest.fixture(scope="module")
def loop(eng):
    """The scene fused from twelve rendered scans: dict(source, fused meshes, volume, the scans' vertex images, poses)."""
    from overlapnet_amd import tsdf
    from overlapnet_amd.mesh import TriangleMesh
    v, t = R.scene(0)
    source = TriangleMesh(v, t)
    poses = R.scene_poses(15)
    r = eng.render_scans(source, poses[:12], BUILD_HW[0], BUILD_HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range", "vertex"))
    lo, hi = v.min(axis=0).astype(np.float64) - 1.0, v.max(axis=0).astype(np.float64) + 1.0
    vol = tsdf.TsdfVolume(eng, lo, hi, 0.2, trunc=0.8)
    assert (vol.nx, vol.ny, vol.nz) == (247, 214, 41)
    vol.integrate(r["range"], poses[:12], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE)
    fused = vol.mesh()
    return dict(source=source, fused=fused, vol=vol, lo=lo, hi=hi, poses=poses, vertex=r["vertex"].cpu().numpy(),
                range=r["range"].cpu().numpy())


def test_closed_loop_fused_mesh_renders_like_the_source(eng, loop):
    poses = loop["poses"][12:15]
    a = eng.render_scans(loop["source"], poses, EVAL_HW[0], EVAL_HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range",))["range"]
    b = eng.render_scans(loop["fused"], poses, EVAL_HW[0], EVAL_HW[1], R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE, want=("range",))["range"]
    a, b = a.cpu().numpy(), b.cpu().numpy()
    both, only_src, only_fused = (a > 0) & (b > 0), (a > 0) & ~(b > 0), ~(a > 0) & (b > 0)
    err = np.abs(a - b)[both]
    got = dict(triangles=loop["fused"].n_triangles, both=float(both.mean()), within=float((err <= 0.2).mean()),
               median=float(np.median(err)), fused_only=float(only_fused.mean()), source_only=float(only_src.mean()))
    print("closed loop: " + json.dumps(got))
    assert got["both"] >= 0.80
    assert got["within"] >= 0.80
    assert got["median"] <= 0.10
    assert got["fused_only"] <= 0.03
    assert got["source_only"] <= 0.10


def test_closed_loop_map_from_the_fused_mesh(eng, loop, tmp_path_factory):
    """`OverlapMap.from_mesh` on a 2 m grid inside the room keeps on the fused mesh every pose it keeps on the source mesh, those
    within 1 m of a box or a wall excepted."""
    from tools import synthetic as S
    from overlapnet_amd import localization as L
    from overlapnet_amd.infer import Infer
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07",
           "data_root_folder": str(tmp_path_factory.mktemp("tsdf_map")), "use_depth": True, "use_normals": True,
           "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16,
           "pretrained_weightsfilename": ""}
    g = L.grid_poses((0.0, R.ROOM[0]), (0.0, R.ROOM[1]), 2.0, z=R.SENSOR_Z)
    turn = np.eye(4)
    turn[:3, :3] = R._rot_z(R.SCENE_ROT)
    poses = turn[None] @ g
    xy = g[:, :2, 3]
    blo, bhi = R.scene_boxes(0)
    near = ((xy[:, 0] <= 1.0) | (xy[:, 0] >= R.ROOM[0] - 1.0) | (xy[:, 1] <= 1.0) | (xy[:, 1] >= R.ROOM[1] - 1.0))
    near |= np.any((xy[:, None, 0] >= blo[None, :, 0] - 1.0) & (xy[:, None, 0] <= bhi[None, :, 0] + 1.0) &
                   (xy[:, None, 1] >= blo[None, :, 1] - 1.0) & (xy[:, None, 1] <= bhi[None, :, 1] + 1.0), axis=1)
    infer = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    try:
        kept = {}
        for name in ("source", "fused"):
            infer.feature_volumes = type(infer.feature_volumes)(infer.engine, min_capacity=8)
            m = L.OverlapMap.from_mesh(infer, loop[name], poses, resolution=2.0, max_range=R.MAX_RANGE, min_range=1.0)
            kept[name] = set(int(i) for i in m.kept)
    finally:
        infer.close()
    must = {i for i in kept["source"] if not near[i]}
    print("from_mesh on a 2 m grid: %d poses, source keeps %d, fused keeps %d, %d of the source's lie clear of boxes and walls"
          % (len(poses), len(kept["source"]), len(kept["fused"]), len(must)))
    assert len(must) >= 100
    assert must <= kept["fused"]


def test_integrate_scans_in_chunks(eng, loop):
    """`integrate_scans` on twelve raw scans, five at a time (offset slices that do not start at 0), against one projection of all
    twelve and one `integrate`: the same bits."""
    from overlapnet_amd import tsdf
    clouds = [np.ascontiguousarray(loop["vertex"][s][loop["range"][s] > 0], np.float32) for s in range(12)]
    offsets = np.zeros(13, np.int64)
    offsets[1:] = np.cumsum([c.shape[0] for c in clouds])
    points = np.concatenate(clouds)
    poses = loop["poses"][:12]
    a = tsdf.TsdfVolume(eng, loop["lo"], loop["hi"], 0.2, trunc=0.8)
    a.integrate_scans(points, offsets, poses, proj_h=BUILD_HW[0], proj_w=BUILD_HW[1], fov_up=R.FOV_UP, fov_down=R.FOV_DOWN,
                      max_range=R.MAX_RANGE, chunk=5)
    rng = eng.project(_dev(points), _dev(offsets), int(np.diff(offsets).max()), BUILD_HW[0], BUILD_HW[1], R.FOV_UP, R.FOV_DOWN,
                      R.MAX_RANGE, want=("range",))["range"]
    b = tsdf.TsdfVolume(eng, loop["lo"], loop["hi"], 0.2, trunc=0.8)
    b.integrate(rng, poses, R.FOV_UP, R.FOV_DOWN, R.MAX_RANGE)
    assert a.n_scans == b.n_scans == 12 and bool((b.weight > 0).any())
    assert torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32))
    assert torch.equal(a.weight.view(torch.int32), b.weight.view(torch.int32))


# ---- 8. tools/build_mesh.py end to end ----------------------------------------------------------------------------------------------
def test_build_mesh_tool(loop, tmp_path, capsys):
    from overlapnet_amd.mesh import TriangleMesh
    from tools import build_mesh
    scans = tmp_path / "scans"
    scans.mkdir()
    for s in range(12):
        pts = loop["vertex"][s][loop["range"][s] > 0]                 # the hit pixels' sensor-frame points (x, y, z, 1)
        pts.astype(np.float32).tofile(str(scans / ("%06d.bin" % s)))
    pose_file = tmp_path / "poses.txt"
    with open(pose_file, "w") as f:
        for p in loop["poses"][:12]:
            f.write(" ".join(repr(float(x)) for x in p[:3].reshape(-1)) + "\n")
    cfg = tmp_path / "network.json"
    cfg.write_text(json.dumps({"model": {"inputShape": [BUILD_HW[0], BUILD_HW[1], 4]}}))
    out = tmp_path / "site.ply"
    build_mesh.main(["--config", str(cfg), "--scans", str(scans), "--poses", str(pose_file), "--voxel", "0.2", "--trunc", "0.8",
                     "--max-range", str(R.MAX_RANGE), "--out", str(out), "--chunk", "5",
                     "--bounds"] + [repr(float(x)) for x in np.concatenate([loop["lo"], loop["hi"]])])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    mesh = TriangleMesh.from_ply(str(out))
    print("build_mesh: %d triangles, the fused mesh of the rendered range images has %d" % (mesh.n_triangles, loop["fused"].n_triangles))
    assert line["triangles"] == mesh.n_triangles and line["volume"] == [247, 214, 41]
    assert mesh.n_triangles == loop["fused"].n_triangles
    assert mesh.n_vertices == 3 * mesh.n_triangles
    # without --bounds an oversized volume is refused with the voxel that fits
    with pytest.raises(SystemExit, match="a voxel of"):
        build_mesh.main(["--config", str(cfg), "--scans", str(scans), "--poses", str(pose_file), "--voxel", "0.01", "--out", str(out)])
