"""CPU: the statement of the TSDF fusion and of the extraction (tests/_tsdf_ref.py) checked on its own -- the
float32 statement against the float64 one, marching tetrahedra on analytic volumes -- plus `TriangleMesh.to_ply` and the argument
refusals of `TsdfVolume`.  The GPU tests (tests/test_gpu_tsdf.py) compare the kernels with the same statement."""

import numpy as np
import pytest

import _tsdf_ref as T


# ---- 1. float32 statement against float64 ----------------------------------------------------------------------------------------
def test_f32_statement_against_f64():
    c = T.fused_case("33x17x9")
    f32, f64 = c["f32"], c["f64"]
    touched = f64["updated"].any(axis=0)
    assert touched.mean() > 0.3                                        # the volume is in view
    surface = T.triangles(f32["tsdf"], f32["weight"], c["origin"], T.VOXEL)
    assert surface.shape[0] > 200                                      # and straddles surfaces (a wall and a box)
    amb = f64["ambiguous"]
    share = (amb & touched).sum() / touched.sum()
    print("ambiguous share %.4f of %d updated samples" % (share, touched.sum()))
    assert share <= 0.05
    clear = ~amb
    assert np.array_equal(f32["updated"][:, clear], f64["updated"][:, clear])
    bound = T.error_bound(c["origin"], c["shape"], T.VOXEL, T.TRUNC, c["poses"], 5)
    err = np.abs(f32["tsdf"].astype(np.float64) - f64["tsdf"])[clear].max()
    print("max |tsdf32 - tsdf64| %.3g, bound %.3g" % (err, bound))
    assert err <= bound < 1e-4
    assert np.array_equal(f32["weight"][clear].astype(np.float64), f64["weight"][clear])
    # samples no scan updated stay fresh
    assert np.all(f32["tsdf"][~f32["updated"].any(axis=0)] == 1) and np.all(f32["weight"][~f32["updated"].any(axis=0)] == 0)


def test_statement_in_two_calls_and_saturation():
    c = T.fused_case("33x17x9")
    t0, w0 = T.fresh(c["shape"])
    a = T.integrate(t0, w0, c["origin"], T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"][:2], c["poses"][:2])
    b = T.integrate(a["tsdf"], a["weight"], c["origin"], T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"][2:], c["poses"][2:])
    assert np.array_equal(b["tsdf"], c["f32"]["tsdf"]) and np.array_equal(b["weight"], c["f32"]["weight"])
    same = T.integrate(t0, w0, c["origin"], T.VOXEL, T.TRUNC, 2.0, np.repeat(c["ranges"][:1], 5, 0), np.repeat(c["poses"][:1], 5, 0))
    assert set(np.unique(same["weight"])) == {0.0, 2.0}


# ---- 2. extraction on analytic volumes -------------------------------------------------------------------------------------------
def _edges_bitwise(tri):
    """Every undirected edge of the soup with its count, vertices matched by their float32 bits."""
    bits = np.ascontiguousarray(tri).view(np.uint32).reshape(-1, 3, 3).astype(np.uint64)
    key = (bits[..., 0] << np.uint64(42)) ^ (bits[..., 1] << np.uint64(21)) ^ bits[..., 2]      # per vertex; collisions checked below
    full = [tuple(v) for v in bits.reshape(-1, 3).tolist()]
    assert len({k: None for k in key.reshape(-1).tolist()}) == len(set(full))
    ids = {v: n for n, v in enumerate(sorted(set(full)))}
    vid = np.array([ids[v] for v in full]).reshape(-1, 3)
    count = {}
    for a, b in ((0, 1), (1, 2), (2, 0)):
        for p, q in zip(vid[:, a].tolist(), vid[:, b].tolist()):
            e = (min(p, q), max(p, q))
            count[e] = count.get(e, 0) + 1
    return vid, count


def test_sphere_is_closed_outward_and_crack_free():
    d, w, origin, voxel, centre = T.sphere_volume()
    tri = T.triangles(d, w, origin, voxel)
    assert tri.shape[0] > 1000
    dist = np.linalg.norm(tri.astype(np.float64) - centre, axis=2) / voxel
    assert np.abs(dist - 5.3).max() < 0.5
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    out = (n * (tri.mean(axis=1) - centre)).sum(axis=1)
    area = np.linalg.norm(n, axis=1)
    assert np.all(out[area > 0] > 0)
    vid, count = _edges_bitwise(tri)
    degenerate = (vid[:, 0] == vid[:, 1]) | (vid[:, 1] == vid[:, 2]) | (vid[:, 0] == vid[:, 2])
    assert not degenerate.any()
    assert set(count.values()) == {2}


def test_oblique_plane():
    d, w, origin, voxel, nrm = T.plane_volume()
    tri = T.triangles(d, w, origin, voxel)
    assert tri.shape[0] > 100
    # every vertex on the plane (linear interpolation of a linear field is exact up to rounding), every normal along +nrm
    rel = (tri.astype(np.float64) - origin) / voxel
    assert np.abs(rel @ nrm - 3.1).max() < 1e-4
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    area = np.linalg.norm(n, axis=1)
    assert np.all((n @ nrm)[area > 1e-9] > 0)
    # interior edges are shared by two triangles; an edge on the volume's boundary belongs to one
    _, count = _edges_bitwise(tri[area > 0])
    assert set(count.values()) <= {1, 2}


def test_one_cell_every_sign_pattern():
    origin, voxel = T.ONE_CELL_ORIGIN, T.ONE_CELL_VOXEL
    cases = T.one_cell_volumes()
    assert [c[0] for c in cases] == list(range(1, 255))
    for pattern, inside, d in cases:
        tri = T.triangles(d, np.ones((2, 2, 2), np.float32), origin, voxel)
        want = sum(T.tet_triangle_count([inside[c] for c in tet]) for tet in T.TETS)
        assert tri.shape[0] == want and 1 <= want <= 12, pattern
        assert np.all(tri >= (origin - 1e-6).astype(np.float32)) and np.all(tri <= (origin + voxel + 1e-6).astype(np.float32)), pattern
    for pattern in (0, 255):
        d = np.full((2, 2, 2), -1.0 if pattern else 1.0, np.float32)
        assert T.triangles(d, np.ones((2, 2, 2), np.float32), origin, voxel).shape[0] == 0


def test_tet_orientation_of_single_corner_cases():
    """One inside corner: its triangles' normals point away from it."""
    origin, voxel = np.zeros(3), 1.0
    for c in range(8):
        d = np.ones(8, np.float32)
        d[c] = -1
        tri = T.triangles(d.reshape(2, 2, 2), np.ones((2, 2, 2), np.float32), origin, voxel)
        corner = np.array([c & 1, (c >> 1) & 1, c >> 2], float)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert tri.shape[0] >= 1 and np.all(((tri.mean(axis=1) - corner) * n).sum(axis=1) > 0), c
        # and the complement: one outside corner, the normals point towards it
        tri = T.triangles(-d.reshape(2, 2, 2), np.ones((2, 2, 2), np.float32), origin, voxel)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        assert tri.shape[0] >= 1 and np.all(((corner - tri.mean(axis=1)) * n).sum(axis=1) > 0), c


def test_min_weight_kills_the_cells_around_a_corner():
    d, w, origin, voxel, _ = T.plane_volume()
    full = T.triangles(d, w, origin, voxel)
    d, w2, origin, voxel, gone = T.unseen_corner_volume()
    less = T.triangles(d, w2, origin, voxel)
    # the cell of a triangle: the floor of its centroid in voxel units
    cells = np.floor((full.astype(np.float64).mean(axis=1) - origin) / voxel + 1e-9).astype(int)
    keep = np.array([tuple(c) not in gone for c in cells])
    assert keep.sum() < full.shape[0]
    assert np.array_equal(less, full[keep])
    assert np.array_equal(T.triangles(d, w2, origin, voxel, min_weight=0.5), full)


# ---- 3. PLY round trip and TsdfVolume's refusals -----------------------------------------------------------------------------------
def test_to_ply_round_trip(tmp_path):
    from overlapnet_amd.mesh import TriangleMesh
    d, w, origin, voxel, _ = T.sphere_volume()
    tri = T.triangles(d, w, origin, voxel)
    t = tri.shape[0]
    m = TriangleMesh(tri.reshape(-1, 3), np.arange(3 * t, dtype=np.int32).reshape(t, 3))
    path = str(tmp_path / "soup.ply")
    m.to_ply(path)
    back = TriangleMesh.from_ply(path)
    assert back.vertices.dtype == np.float32 and back.triangles.dtype == np.int32
    assert np.array_equal(back.vertices.view(np.uint32), m.vertices.view(np.uint32)) and np.array_equal(back.triangles, m.triangles)
    shared = TriangleMesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 1e-30, 3e38]], np.float32), np.array([[0, 1, 2], [3, 2, 1]]))
    shared.to_ply(path)
    back = TriangleMesh.from_ply(path)
    assert np.array_equal(back.vertices.view(np.uint32), shared.vertices.view(np.uint32)) and np.array_equal(back.triangles, shared.triangles)


class _NoGpu(object):
    """An engine stand-in that fails the test when a refusal comes too late."""
    @property
    def device(self):
        raise AssertionError("the GPU was touched before the arguments were checked")


def test_volume_shape_and_refusals():
    from overlapnet_amd import tsdf
    assert tsdf.volume_shape((0, 0, 0), (6.4, 3.2, 1.6), 0.2) == (33, 17, 9)
    assert tsdf.volume_shape((0, 0, 0), (0.1, 0.1, 0.1), 0.2) == (2, 2, 2)
    assert tsdf.volume_shape((-1, -1, -1), (0.05, 0, 1.01), 0.5) == (4, 3, 6)
    bad = [dict(lo=(0, 0), hi=(1, 1, 1), voxel=0.1), dict(lo=(0, 0, 0), hi=(1, 0, 1), voxel=0.1),
           dict(lo=(0, 0, 0), hi=(1, np.nan, 1), voxel=0.1), dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.0),
           dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=-1.0), dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=float("nan")),
           dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, trunc=0.0), dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, trunc=float("nan")),
           dict(lo=(0, 0, 0), hi=(1, 1, 1), voxel=0.1, max_weight=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            tsdf.TsdfVolume(_NoGpu(), **kw)
    with pytest.raises(ValueError, match=r"a voxel of 0\.\d+ m fits") as e:
        tsdf.TsdfVolume(_NoGpu(), (0, 0, 0), (200, 200, 20), 0.02)
    fit = float(str(e.value).split("a voxel of ")[1].split(" m fits")[0])
    assert np.prod(tsdf.volume_shape((0, 0, 0), (200, 200, 20), fit)) <= tsdf.MAX_SAMPLES < np.prod(
        [np.ceil(x / (fit * 0.9)) + 1 for x in (200, 200, 20)])


def test_integrate_refusals_before_the_gpu():
    from overlapnet_amd import tsdf
    vol = tsdf.TsdfVolume.__new__(tsdf.TsdfVolume)
    vol.engine = _NoGpu()
    vol.n_scans = 0
    poses = np.tile(np.eye(4), (2, 1, 1))
    for kw in (dict(range_images=np.zeros((2, 4)), poses=poses), dict(range_images=np.zeros((2, 4, 8)), poses=poses[:1]),
               dict(range_images=np.zeros((2, 0, 8)), poses=poses), dict(range_images=np.zeros((2, 4, 8)), poses=poses, max_range=0.0),
               dict(range_images=np.zeros((2, 4, 8)), poses=poses, max_range=float("nan"))):
        with pytest.raises(ValueError):
            vol.integrate(**kw)
    pts = np.zeros((10, 4), np.float32)
    for kw in (dict(points=pts, offsets=[0, 5, 10], poses=poses[:1]), dict(points=pts, offsets=[0, 5, 11], poses=poses),
               dict(points=pts, offsets=[0, 6, 5], poses=poses), dict(points=pts, offsets=[0, 5, 10], poses=poses, chunk=0)):
        with pytest.raises(ValueError):
            vol.integrate_scans(**kw)
    with pytest.raises(ValueError):
        vol.mesh(min_weight=float("nan"))
