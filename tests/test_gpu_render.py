"""GPU (MI355X): `ovn_render_scans` (csrc/render_mesh.hip) -- the exhaustive route against the NumPy float32 statement of the renderer
(tests/_render_ref.py) BIT FOR BIT, the hierarchy route against the exhaustive one, the tie rule, the round trip through the projection,
normals and stacking, batch independence, every refusal, and `OverlapMap.from_mesh` end to end.

Hierarchy against exhaustive: the target is every pixel.  A differing pixel is tolerated only where the float64 reference marks the
pixel ambiguous (_render_ref.render(..., ambiguous=True): a candidate triangle within 1e-4 of an edge, nearly edge-on, or within 1 mm
of max_range); each case prints its count, DESIGN.md section 28 records them (all 0 when this was written)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _render_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

SHAPES = [(16, 90), (5, 67), (64, 900)]
OVN_ERR_ARG = 1
SENSOR = dict(fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE)


@pytest.fixture(scope="module")
def eng():
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(64, 900, 4, device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scene():
    return R.scene(0)


@pytest.fixture(scope="module")
def mesh(scene):
    from overlapnet_amd.mesh import TriangleMesh
    return TriangleMesh(*scene)


def _poses(shape):
    """Inside the room (two for 64 x 900, three for the small shapes), then one outside looking at a wall, one far away."""
    inside = R.scene_poses(2 if shape == (64, 900) else 3, seed=shape[0])
    return np.concatenate([inside, R.pose_at(-6.0, 15.0, 1.7, 0.2)[None], R.pose_at(5000.0, -7000.0, 1.7, 1.0)[None]])


_REF = {}


def _ref32(scene, shape):
    """The float32 statement for the inside poses of `shape`, computed once."""
    if shape not in _REF:
        n_in = 2 if shape == (64, 900) else 3
        _REF[shape] = R.render(scene[0], scene[1], _poses(shape)[:n_in], shape[0], shape[1], np.float32)
    return _REF[shape]


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _render(eng, mesh, poses, shape, want=("range", "tri_id"), **kw):
    return eng.render_scans(mesh, poses, shape[0], shape[1], want=want, **dict(SENSOR, **kw))


# ---- exhaustive route against the float32 statement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_exhaustive_matches_the_float32_statement_bit_for_bit(eng, mesh, scene, shape):
    ref = _ref32(scene, shape)
    n_in = ref["range"].shape[0]
    got = _render(eng, mesh, _poses(shape)[:n_in], shape, want=("range", "tri_id", "vertex"), exhaustive=True)
    rng, tid, vtx = got["range"].cpu().numpy(), got["tri_id"].cpu().numpy(), got["vertex"].cpu().numpy()
    print("shape %s: %d pixels, %d range words differ, %d ids differ, hit fraction %.3f"
          % (shape, rng.size, int((rng.view(np.int32) != ref["range"].view(np.int32)).sum()), int((tid != ref["tri_id"]).sum()),
             float((tid >= 0).mean())))
    assert np.array_equal(tid, ref["tri_id"])
    assert np.array_equal(rng.view(np.int32), ref["range"].view(np.int32))
    assert np.array_equal(vtx.view(np.int32), ref["vertex"].view(np.int32))
    assert 0.5 < (tid >= 0).mean() < 0.99


# ---- hierarchy route against the exhaustive route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5, 936])
@pytest.mark.parametrize("shape", SHAPES)
def test_hierarchy_matches_exhaustive(eng, scene, shape, T):
    from overlapnet_amd.mesh import TriangleMesh
    v, t = scene
    # T = 1 and 5: floor triangles under the first pose, so that they are seen
    sub = TriangleMesh(v, t[:T])
    poses = _poses(shape)
    if T < 936:
        c = v[t[:T]].reshape(-1, 3).mean(axis=0)
        poses = np.concatenate([poses, np.eye(4)[None]])
        poses[-1, :3, 3] = c + np.array([0.3, -0.2, 0.5])
    a = _render(eng, sub, poses, shape, exhaustive=True)
    b = _render(eng, sub, poses, shape)
    differ = (_bits(a["range"]) != _bits(b["range"])) | (_bits(a["tri_id"]) != _bits(b["tri_id"]))
    hits = int((a["tri_id"] >= 0).sum().item())
    print("shape %s T %d: %d poses, %d hit pixels, %d pixels differ between the routes" % (shape, T, len(poses), hits, int(differ.sum())))
    assert hits > 0
    assert int((a["tri_id"][-2 if T < 936 else -1] >= 0).sum().item()) == 0        # the far pose sees nothing
    if differ.any():
        amb = R.render(v, t[:T], poses, shape[0], shape[1], np.float64, ambiguous=True)["ambiguous"]
        assert not np.any(differ & ~amb), "%d pixels differ where the reference is not ambiguous" % int((differ & ~amb).sum())
    else:
        assert torch.equal(a["range"], b["range"]) and torch.equal(a["tri_id"], b["tri_id"])


def test_equal_t_goes_to_the_smaller_index(eng, scene):
    from overlapnet_amd.mesh import TriangleMesh
    v, t = scene
    # every triangle twice, the copies FIRST in the hierarchy's leaves or last: either way the lower index must be reported
    for tris in (np.concatenate([t, t]), np.concatenate([t, t[::-1]])):
        dup = TriangleMesh(v, tris)
        poses = _poses((16, 90))
        one = _render(eng, TriangleMesh(v, t), poses, (16, 90), exhaustive=True)
        for exhaustive in (True, False):
            r = _render(eng, dup, poses, (16, 90), exhaustive=exhaustive)
            assert int(r["tri_id"].max().item()) < 936
            assert torch.equal(r["range"], one["range"]) and torch.equal(r["tri_id"], one["tri_id"])


# ---- round trip through the projection ----------------------------------------------------------------------------------------------
def test_round_trip_through_project_scans(eng, mesh):
    from overlapnet_amd.preprocess import project_scans
    pose = _poses((64, 900))[:1]
    r = _render(eng, mesh, pose, (64, 900), want=("range", "vertex"))
    rng, vtx = r["range"][0].cpu().numpy(), r["vertex"][0].cpu().numpy()
    valid = rng > 0
    cloud = vtx[valid]                                             # (N,4), row-major pixel order
    assert np.all(cloud[:, 3] == 1) and cloud.shape[0] > 0.5 * valid.size
    p = project_scans([cloud], engine=eng, proj_H=64, proj_W=900, fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE,
                      want=("range", "idx"))
    prng, pidx = p["range"][0].cpu().numpy(), p["idx"][0].cpu().numpy()
    assert np.array_equal(prng > 0, valid)                         # the occupancy mask
    assert np.array_equal(pidx[valid], np.arange(cloud.shape[0]))  # every point in its own pixel
    ulp = np.abs(prng[valid].view(np.int32).astype(np.int64) - rng[valid].view(np.int32).astype(np.int64))
    print("round trip: %d points, projected range within %d ulp of t" % (cloud.shape[0], int(ulp.max())))
    assert ulp.max() <= 16


# ---- normals and stacking -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 67), (64, 900)])
def test_normals_and_stacked_are_the_projection_kernels(eng, mesh, shape):
    poses = _poses(shape)[:3]
    full = _render(eng, mesh, poses, shape, want=("range", "vertex", "normal"), stacked_flags=(True, True))
    nrm = eng.normals(full["range"], full["vertex"])
    assert torch.equal(full["normal"].view(torch.int32), nrm.view(torch.int32))
    assert bool((nrm[full["range"] > 0] != -1).any())
    d = full["range"].unsqueeze(-1)
    for flags, want in (((True, True), torch.cat([d, nrm], -1)), ((True, False), d), ((False, True), nrm)):
        # with and without the images the normals are made from among the outputs (else they live in the library's scratch)
        for outs in (("range", "vertex"), ()):
            s = _render(eng, mesh, poses, shape, want=outs, stacked_flags=flags)["stacked"]
            assert s.shape == want.shape and torch.equal(s.view(torch.int32), want.contiguous().view(torch.int32))
    only = _render(eng, mesh, poses, shape, want=("normal",))
    assert set(only) == {"normal"} and torch.equal(only["normal"].view(torch.int32), nrm.view(torch.int32))


# ---- same bits ----------------------------------------------------------------------------------------------------------------------
def test_a_pose_renders_alone_as_in_any_batch_and_twice_alike(eng, mesh):
    shape = (16, 90)
    poses = _poses(shape)
    for exhaustive in (False, True):
        batch = _render(eng, mesh, poses, shape, want=("range", "tri_id", "vertex", "normal"), exhaustive=exhaustive)
        again = _render(eng, mesh, poses, shape, want=("range", "tri_id", "vertex", "normal"), exhaustive=exhaustive)
        rev = _render(eng, mesh, poses[::-1].copy(), shape, want=("range", "tri_id", "vertex", "normal"), exhaustive=exhaustive)
        for k in batch:
            assert torch.equal(batch[k].view(torch.int32), again[k].view(torch.int32))
            assert torch.equal(batch[k].view(torch.int32), rev[k].flip(0).view(torch.int32))
        for i in range(len(poses)):
            alone = _render(eng, mesh, poses[i:i + 1], shape, want=("range", "tri_id", "vertex", "normal"), exhaustive=exhaustive)
            for k in batch:
                assert torch.equal(batch[k][i].view(torch.int32), alone[k][0].view(torch.int32))


def test_non_finite_pose_gives_an_empty_scan(eng, mesh):
    poses = _poses((16, 90))[:2]
    poses[1, 1, 3] = np.inf
    for exhaustive in (False, True):
        r = _render(eng, mesh, poses, (16, 90), want=("range", "tri_id", "vertex"), exhaustive=exhaustive)
        assert bool((r["tri_id"][0] >= 0).any())
        assert bool((r["tri_id"][1] == -1).all()) and bool((r["range"][1] == -1).all()) and bool((r["vertex"][1] == -1).all())


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched(eng, mesh):
    from overlapnet_amd.engine import _ptr
    from overlapnet_amd.mesh import direction_tables
    H, W, n = 8, 16, 2
    dev = eng.device
    md = mesh.device(eng)
    poses = torch.from_numpy(_poses((16, 90))[:n].copy()).to(dev)
    tabs = [torch.from_numpy(t).to(dev) for t in direction_tables(H, W, R.FOV_UP, R.FOV_DOWN)]
    outs = dict(range=torch.full((n, H, W), 7.0, device=dev), tri_id=torch.full((n, H, W), 7, dtype=torch.int32, device=dev),
                vertex=torch.full((n, H, W, 4), 7.0, device=dev), normal=torch.full((n, H, W, 3), 7.0, device=dev),
                stacked=torch.full((n, H, W, 4), 7.0, device=dev))
    base = dict(vertices=md["vertices"], V=mesh.n_vertices, triangles=md["triangles"], T=mesh.n_triangles, nodes=md["nodes"],
                order=md["order"], leaves=md["leaves"], poses=poses, n=n, H=H, W=W, max_range=20.0, ud=1, un=1, ui=0, us=0)

    def call(**over):
        a = dict(base, **over)
        return eng.lib.ovn_render_scans(eng._h, _ptr(a["vertices"]), a["V"], _ptr(a["triangles"]), a["T"], _ptr(a["nodes"]),
                                        _ptr(a["order"]), a["leaves"], _ptr(a["poses"]), a["n"], a["H"], a["W"], _ptr(tabs[0]),
                                        _ptr(tabs[1]), _ptr(tabs[2]), _ptr(tabs[3]), a["max_range"], _ptr(outs["range"]),
                                        _ptr(outs["tri_id"]), _ptr(outs["vertex"]), _ptr(outs["normal"]), _ptr(outs["stacked"]),
                                        a["ud"], a["un"], a["ui"], a["us"], eng._stream())

    refused = [dict(T=0), dict(T=-3), dict(T=(1 << 27) + 1), dict(V=0), dict(H=0), dict(W=-1), dict(H=65536, W=65536),
               dict(H=46341, W=46341), dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=float("nan")), dict(vertices=None),
               dict(triangles=None), dict(poses=None), dict(ui=1), dict(us=1), dict(ud=0, un=0), dict(n=-1), dict(nodes=None),
               dict(order=None), dict(leaves=255), dict(leaves=128), dict(leaves=0)]
    for over in refused:
        assert call(**over) == OVN_ERR_ARG, over
        assert eng.lib.ovn_last_error()
    assert call(n=0) == 0                                           # a no-op
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 7).all()), k
    assert call() == 0                                              # and the same arguments, unrefused, do write
    torch.cuda.synchronize()
    assert bool((outs["range"] != 7).all()) and bool((outs["stacked"] != 7).all())
    # the engine's wrapper passes the flags through: a rendered scan has no intensity and no class probabilities
    from overlapnet_amd._lib import OvnError
    for flags in ((True, True, True), (True, True, False, True)):
        with pytest.raises(OvnError, match="no intensity"):
            eng.render_scans(mesh, poses, H, W, stacked_flags=flags, **SENSOR)
    with pytest.raises(OvnError, match="no output"):
        eng.render_scans(mesh, poses, H, W, want=("intensity",), **SENSOR)


# ---- OverlapMap.from_mesh -----------------------------------------------------------------------------------------------------------
PILLAR = (np.array([20.0, 12.5, 0.0]), np.array([21.0, 13.5, 3.0]))     # room frame; two of the eight grid cells lie inside it
MIN_RANGE = 1.0


def _map_mesh(scene):
    """The scene plus a closed 1 x 1 x 3 m pillar.  On a two-sided mesh a sensor inside a closed box sees the box from inside in every
    pixel, so the valid-pixel rule alone keeps it; with the blind zone of a real sensor (min_range = 1 m) nearly all of those hits
    vanish and the pose is dropped."""
    from overlapnet_amd.mesh import TriangleMesh
    v, t = scene
    parts = [R._grid_quads(*f, 2, 2) for f in R._box_faces(*PILLAR)]
    vs, ts, base = [v], [t], v.shape[0]
    for p, q in parts:
        vs.append((p @ R._rot_z(R.SCENE_ROT).T).astype(np.float32))
        ts.append((q + base).astype(np.int32))
        base += p.shape[0]
    return TriangleMesh(np.concatenate(vs), np.concatenate(ts))


def _map_poses():
    """Eight grid poses (4 x 2 cells of 0.5 m) laid in the ROOM's frame and moved into the scene's."""
    from overlapnet_amd.localization import grid_poses
    g = grid_poses((19.5, 21.5), (12.0, 13.0), 0.5, z=R.SENSOR_Z)
    assert g.shape[0] == 8
    turn = np.eye(4)
    turn[:3, :3] = R._rot_z(R.SCENE_ROT)
    return turn[None] @ g


INSIDE = [5, 6]        # cells (20.25, 12.75) and (20.75, 12.75)


@pytest.fixture(scope="module")
def world(scene, tmp_path_factory):
    from tools import synthetic as S
    from overlapnet_amd.infer import Infer
    cfg = {"model": dict(S.REFERENCE_MODEL_CFG, inputShape=[64, 900]), "infer_seqs": "07",
           "data_root_folder": str(tmp_path_factory.mktemp("render_map")), "use_depth": True, "use_normals": True,
           "use_class_probabilities": False, "use_class_probabilities_pca": False, "use_intensity": False, "batch_size": 16,
           "pretrained_weightsfilename": ""}
    infer = Infer(cfg, weights=S.make_test_weights(4, seed=0))
    yield dict(infer=infer, cfg=cfg, mesh=_map_mesh(scene), poses=_map_poses())
    infer.close()


def test_from_mesh_end_to_end(world, tmp_path):
    from overlapnet_amd import localization as L
    infer, mesh, poses = world["infer"], world["mesh"], world["poses"]
    eng = infer.engine
    infer.feature_volumes = type(infer.feature_volumes)(eng, min_capacity=8)
    mp = L.OverlapMap.from_mesh(infer, mesh, poses, resolution=0.5, chunk=3, max_range=R.MAX_RANGE, min_range=MIN_RANGE)
    kept = [i for i in range(8) if i not in INSIDE]
    assert mp.mesh_built and list(mp.kept) == kept and mp.n_frames == 6 and len(infer.feature_volumes) == 6
    # without the blind zone the two poses inside the pillar see its inside everywhere and stay
    counts = (eng.render_scans(mesh, poses, 64, 900, max_range=R.MAX_RANGE, want=("range",))["range"] > 0).sum(dim=(1, 2)).cpu().numpy()
    assert np.all(counts[INSIDE] > 0.9 * 64 * 900)
    # the cached volume of every kept pose is the leg of that pose rendered alone
    feats = infer.feature_volumes.device_features
    for slot, i in enumerate(kept):
        alone = eng.render_scans(mesh, poses[i:i + 1], 64, 900, max_range=R.MAX_RANGE, want=(), stacked_flags=(True, True))["stacked"]
        assert torch.equal(feats[slot], eng.leg(alone)[0])
    xy = L.poses_xyyaw(poses[kept])[:, :2]
    assert np.array_equal(mp.cell_frame_host, L.build_cell_frame(xy, mp.origin_x, mp.origin_y, 0.5, mp.nx, mp.ny, 0.5))
    assert np.allclose(mp.poses, L.poses_xyyaw(poses[kept]))
    # save / load round trip (load renders the kept poses again from the mesh it is given)
    path = str(tmp_path / "map.npz")
    mp.save(path)
    before = feats.clone()
    with pytest.raises(L.OvnError, match="mesh"):
        L.OverlapMap.load(infer, path)
    infer.feature_volumes = type(infer.feature_volumes)(eng, min_capacity=8)
    m2 = L.OverlapMap.load(infer, path, mesh)
    assert m2.mesh_built and list(m2.kept) == kept and m2.frame_names == mp.frame_names
    assert np.array_equal(m2.poses, mp.poses) and np.array_equal(m2.cell_frame_host, mp.cell_frame_host)
    assert (m2.resolution, m2.reach, m2.sensor, m2.min_range) == (mp.resolution, mp.reach, mp.sensor, mp.min_range)
    assert torch.equal(infer.feature_volumes.device_features, before)
    # one localization step with a query rendered from the same mesh
    q = eng.render_scans(mesh, poses[kept[2]:kept[2] + 1], 64, 900, max_range=R.MAX_RANGE, want=(), stacked_flags=(True, True))
    loc = L.MonteCarloLocalizer(m2, 256, seed=1)
    est = loc.step(q["stacked"], (0.0, 0.0, 0.0), (0.05, 0.05, 0.01))
    assert np.isfinite([est.x, est.y, est.yaw, est.n_eff]).all() and est.frames_scored >= 1
    assert mp.origin_x <= est.x <= mp.origin_x + mp.nx * 0.5 and mp.origin_y <= est.y <= mp.origin_y + mp.ny * 0.5


def test_from_mesh_refuses_what_a_rendered_scan_lacks(world):
    from overlapnet_amd import localization as L
    infer, mesh, poses = world["infer"], world["mesh"], world["poses"]
    infer.feature_volumes = type(infer.feature_volumes)(infer.engine, min_capacity=8)
    infer.use_intensity = True
    try:
        with pytest.raises(L.OvnError, match="intensity"):
            L.OverlapMap.from_mesh(infer, mesh, poses, resolution=0.5)
    finally:
        infer.use_intensity = False
    with pytest.raises(L.OvnError, match="none of the"):
        far = poses.copy()
        far[:, 0, 3] += 1e4
        L.OverlapMap.from_mesh(infer, mesh, far, resolution=0.5)
    assert len(infer.feature_volumes) == 0

    class Sharded(object):
        _world = 2
    with pytest.raises(L.OvnError, match="sharded"):
        L.OverlapMap.from_mesh(Sharded(), mesh, poses, resolution=0.5)
