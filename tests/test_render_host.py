"""CPU: the host side of `ovn_render_scans` -- the float32 statement of the renderer against its float64 reference
(tests/_render_ref.py), the bounding-volume hierarchy of overlapnet_amd/mesh.py, the PLY reader, `grid_poses`, the drop rule of
`OverlapMap.from_mesh`, and the export's presence in header, library and binding.

The float32 / float64 comparison leaves out the pixels the float64 reference marks ambiguous (a candidate triangle within 1e-4 of an
edge, nearly edge-on, or within 1 mm of max_range), at most 0.5 % of all pixels.  Measured with the scene of _render_ref.scene(0) on six
poses at 16 x 90: 0.081 % ambiguous, no hit/miss or index mismatch on the rest, largest |t32 - t64| 1.14e-5 m (the test prints the
figures of its run).  The assertion is |t32 - t64| < 1e-4 m: a tenth of the 1 mm the ambiguity margins assume."""
import os
import re
import struct

import numpy as np
import pytest

import _render_ref as R
from overlapnet_amd import _lib, localization as L
from overlapnet_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_BOUND = 1e-4
AMBIGUOUS_MAX = 0.005


@pytest.fixture(scope="module")
def scene():
    return R.scene(0)


def test_scene_has_936_triangles_over_its_own_vertices(scene):
    v, t = scene
    assert t.shape == (936, 3) and t.dtype == np.int32 and v.dtype == np.float32
    assert t.min() == 0 and t.max() == v.shape[0] - 1


def test_float32_statement_against_float64(scene):
    v, t = scene
    poses = R.scene_poses(6, 0)
    r32 = R.render(v, t, poses, 16, 90, np.float32)
    r64 = R.render(v, t, poses, 16, 90, np.float64, ambiguous=True)
    amb = r64["ambiguous"]
    frac = amb.mean()
    clear = ~amb
    hit32, hit64 = r32["tri_id"] >= 0, r64["tri_id"] >= 0
    miss = 1.0 - hit64.mean()
    both = clear & hit32 & hit64
    dt = np.abs(r32["range"][both].astype(np.float64) - r64["range"][both]).max()
    print("ambiguous %.3f %% of %d pixels, misses %.1f %%, hit/miss mismatches %d, index mismatches %d, max |t32 - t64| %.3g m"
          % (100 * frac, amb.size, 100 * miss, int((hit32 != hit64)[clear].sum()),
             int((r32["tri_id"] != r64["tri_id"])[clear].sum()), dt))
    assert frac <= AMBIGUOUS_MAX
    assert 0.01 < miss < 0.5                         # some rays leave through the open top or end beyond max_range
    assert np.array_equal(hit32[clear], hit64[clear])
    assert np.array_equal(r32["tri_id"][clear], r64["tri_id"][clear])
    assert dt < T_BOUND
    # the vertex image is t d_s with the project convention
    assert np.all(r32["vertex"][~hit32] == -1) and np.all(r32["vertex"][hit32][:, 3] == 1)
    assert r32["range"].dtype == np.float32 and np.all(r32["range"][~hit32] == -1)
    assert np.all(r32["range"][hit32] < np.float32(R.MAX_RANGE))


def test_non_finite_pose_and_bad_triangle_are_skipped(scene):
    v, t = scene
    poses = R.scene_poses(2, 0)
    poses[1, 0, 3] = np.nan
    r = R.render(v, t, poses, 5, 9, np.float32)
    assert np.all(r["tri_id"][1] == -1) and np.any(r["tri_id"][0] >= 0)
    t2 = t.copy()
    t2[::2, 1] = v.shape[0]                           # every other triangle names a vertex that does not exist
    r2 = R.render(v, t2, poses[:1], 5, 9, np.float32)
    assert not np.any(r2["tri_id"][r2["tri_id"] >= 0] % 2 == 0)


# ---- the hierarchy -----------------------------------------------------------------------------------------------------------------
def _check_bvh(v, t):
    nodes, order, nl = M.build_bvh(v, t)
    T = t.shape[0]
    assert nl >= 1 and nl & (nl - 1) == 0 and nl * M.LEAF_TRIANGLES >= T and (nl == 1 or (nl // 2) * M.LEAF_TRIANGLES < T)
    assert nodes.shape == (2 * nl, 8) and nodes.dtype == np.float32 and order.dtype == np.int32
    assert np.array_equal(np.sort(order), np.arange(T))            # every triangle in exactly one leaf slot
    lo, hi = nodes[:, 0:3], nodes[:, 4:7]
    pad = M.box_padding(v)
    assert pad > 0
    corners = v[t[order]]                                         # (T,3,3) in leaf order
    for j in range(nl):
        c = corners[j * M.LEAF_TRIANGLES:(j + 1) * M.LEAF_TRIANGLES].reshape(-1, 3).astype(np.float64)
        if c.shape[0] == 0:
            assert lo[nl + j, 0] > hi[nl + j, 0]                   # an empty leaf says so
            continue
        assert np.all(lo[nl + j].astype(np.float64) <= c.min(axis=0) - pad)      # padded by at least `pad`
        assert np.all(hi[nl + j].astype(np.float64) >= c.max(axis=0) + pad)
    for i in range(1, nl):                                         # every inner box contains its children's boxes
        for ch in (2 * i, 2 * i + 1):
            if lo[ch, 0] > hi[ch, 0]:
                continue
            assert np.all(lo[i] <= lo[ch]) and np.all(hi[i] >= hi[ch])
    return nodes, order, nl


def test_bvh_of_the_scene(scene):
    v, t = scene
    nodes, order, nl = _check_bvh(v, t)
    assert nl == 256
    # Morton order keeps a leaf compact: the median leaf box is far smaller than the room
    full = nodes[nl:, 0] <= nodes[nl:, 4]
    ext = (nodes[nl:, 4:7][full] - nodes[nl:, 0:3][full]).max(axis=1)
    assert full.sum() == 234 and np.median(ext) < 12.0


@pytest.mark.parametrize("T", [1, 5])
def test_bvh_of_tiny_meshes(scene, T):
    v, t = scene
    nodes, order, nl = _check_bvh(v, t[:T])
    assert nl == (1 if T == 1 else 2)


def test_bvh_when_all_centroids_coincide():
    # 9 triangles of different sizes around one centroid: every Morton code is equal, the stable sort keeps the index order
    g = np.random.default_rng(3)
    base = np.array([[1.0, 0.0, 0.0], [-0.5, 0.75, 0.0], [-0.5, -0.75, 0.0]])
    v = np.concatenate([(k + 1.0) * base + np.array([2.0, 3.0, 1.0]) for k in range(9)]).astype(np.float32)
    t = np.arange(27, dtype=np.int32).reshape(9, 3)
    nodes, order, nl = _check_bvh(v, t)
    assert nl == 4 and np.array_equal(order, np.arange(9))
    del g


def test_morton_codes():
    p = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    c = M.morton30(p)
    assert c[0] == 0 and c[1] == (1 << 30) - 1
    assert c[2] == int("100" * 10, 2) and c[3] == int("010" * 10, 2) and c[4] == int("001" * 10, 2)
    assert np.all(M.morton30(np.ones((3, 3))) == 0)


def test_direction_tables_are_pixel_centres():
    ca, sa, cp, sp = M.direction_tables(64, 900, 3.0, -25.0)
    assert ca.dtype == np.float32 and ca.shape == (900,) and cp.shape == (64,)
    # inverting range_projection's formulas at the ray of pixel (py, px) gives py + 0.5, px + 0.5
    yaw = -np.arctan2(sa.astype(np.float64), ca.astype(np.float64))
    px = 0.5 * (yaw / np.pi + 1.0) * 900
    assert np.abs(px - (np.arange(900) + 0.5)).max() < 1e-4
    fov = (3.0 + 25.0) / 180 * np.pi
    py = (1.0 - (np.arcsin(sp.astype(np.float64)) + 25.0 / 180 * np.pi) / fov) * 64
    assert np.abs(py - (np.arange(64) + 0.5)).max() < 1e-4


# ---- mesh validation and the PLY reader ---------------------------------------------------------------------------------------------
def test_triangle_mesh_validates(scene):
    v, t = scene
    m = M.TriangleMesh(v.astype(np.float64), t.astype(np.int64))
    assert m.vertices.dtype == np.float32 and m.triangles.dtype == np.int32 and m.n_triangles == 936
    assert m._bvh is None and m.bvh[2] == 256 and m._bvh is not None          # lazy
    bad = v.copy()
    bad[3, 1] = np.inf
    for args in ((bad, t), (v, t[:0]), (v[:, :2], t), (v, t[:, :2]), (v, t.astype(np.float32)), (v.astype(np.int32), t)):
        with pytest.raises(ValueError):
            M.TriangleMesh(*args)
    t2 = t.copy()
    t2[5, 2] = v.shape[0]
    with pytest.raises(ValueError, match="outside"):
        M.TriangleMesh(v, t2)
    t2[5, 2] = -1
    with pytest.raises(ValueError, match="outside"):
        M.TriangleMesh(v, t2)


def _write_ply(path, v, t, fmt, extra_vertex_prop=False, face_counts=None, index_type="int"):
    vprops = "property float x\nproperty float y\nproperty float z\n" + ("property uchar red\n" if extra_vertex_prop else "")
    head = ("ply\nformat %s 1.0\ncomment written by the test\nelement vertex %d\n%selement face %d\n"
            "property list uchar %s vertex_indices\nend_header\n" % (fmt, v.shape[0], vprops, t.shape[0], index_type))
    counts = face_counts if face_counts is not None else [3] * t.shape[0]
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        if fmt == "ascii":
            for p in v:
                fh.write(("%r %r %r%s\n" % (float(p[0]), float(p[1]), float(p[2]), " 7" if extra_vertex_prop else "")).encode())
            for c, f in zip(counts, t):
                fh.write(("%d %s\n" % (c, " ".join(str(int(i)) for i in f[:c]))).encode())
        else:
            for p in v:
                fh.write(struct.pack("<fff", *[float(x) for x in p]) + (b"\x07" if extra_vertex_prop else b""))
            code = {"int": "<i", "uint": "<I", "ushort": "<H"}[index_type]
            for c, f in zip(counts, t):
                fh.write(struct.pack("<B", c) + b"".join(struct.pack(code, int(i)) for i in f[:c]))


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
@pytest.mark.parametrize("extra", [False, True])
def test_ply_round_trip(tmp_path, scene, fmt, extra):
    v, t = scene
    path = str(tmp_path / "m.ply")
    _write_ply(path, v[:200], t[:40] % 200, fmt, extra_vertex_prop=extra, index_type="uint" if extra else "int")
    m = M.TriangleMesh.from_ply(path)
    assert np.array_equal(m.vertices, v[:200]) and np.array_equal(m.triangles, t[:40] % 200)


def test_malformed_ply_raises(tmp_path, scene):
    v, t = scene
    v, t = v[:50], t[:10] % 50
    p = str(tmp_path / "bad.ply")
    quad = np.concatenate([t, t[:, :1]], axis=1)
    for fmt in ("ascii", "binary_little_endian"):
        _write_ply(p, v, quad, fmt, face_counts=[3] * 9 + [4])
        with pytest.raises(ValueError, match="4 vertices"):
            M.TriangleMesh.from_ply(p)
        _write_ply(p, v, t, fmt)
        data = open(p, "rb").read()
        open(p, "wb").write(data[:-5])                                       # truncated
        with pytest.raises(ValueError):
            M.TriangleMesh.from_ply(p)
        open(p, "wb").write(data.replace(b"format %s" % fmt.encode(), b"format binary_big_endian"))
        with pytest.raises(ValueError, match="binary_big_endian"):
            M.TriangleMesh.from_ply(p)
        open(p, "wb").write(data.replace(b"property float z\n", b""))
        with pytest.raises(ValueError, match="x, y or z"):
            M.TriangleMesh.from_ply(p)
        open(p, "wb").write(data.replace(b"element face", b"element edge"))
        with pytest.raises(ValueError, match="edge"):
            M.TriangleMesh.from_ply(p)
    open(p, "wb").write(b"solid not a ply\n")
    with pytest.raises(ValueError, match="not a PLY"):
        M.TriangleMesh.from_ply(p)
    _write_ply(p, v, t + 45, "ascii")                                        # indices past the last vertex
    with pytest.raises(ValueError, match="outside"):
        M.TriangleMesh.from_ply(p)


def test_obj_reader(tmp_path, scene):
    v, t = scene
    p = str(tmp_path / "m.obj")
    with open(p, "w") as fh:
        fh.write("# comment\n")
        for q in v[:30]:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in q))
        for f in t[:8] % 30:
            fh.write("f %d/1/1 %d/2/2 %d\n" % tuple(int(i) + 1 for i in f))
    m = M.TriangleMesh.from_obj(p)
    assert np.array_equal(m.vertices, v[:30]) and np.array_equal(m.triangles, t[:8] % 30)


# ---- grid poses and the drop rule ---------------------------------------------------------------------------------------------------
def test_grid_poses():
    p = L.grid_poses((2.0, 5.0), (-1.0, 1.0), 1.0, z=1.7, yaw=0.5)
    assert p.shape == (6, 4, 4) and p.dtype == np.float64
    assert np.allclose(p[:, 0, 3], [2.5, 3.5, 4.5, 2.5, 3.5, 4.5]) and np.allclose(p[:, 1, 3], [-0.5] * 3 + [0.5] * 3)
    assert np.all(p[:, 2, 3] == 1.7) and np.all(p[:, 3] == [0, 0, 0, 1])
    assert np.allclose(L.poses_xyyaw(p)[:, 2], 0.5)
    assert np.allclose(p[0, :3, :3] @ p[0, :3, :3].T, np.eye(3))
    assert L.grid_poses((0.0, 0.2), (0.0, 0.0), 1.0, z=0.0).shape == (1, 4, 4)
    assert L.grid_poses((0.0, 2.5), (0.0, 1.0), 1.0, z=0.0).shape == (3, 4, 4)
    with pytest.raises(ValueError):
        L.grid_poses((0.0, 1.0), (0.0, 1.0), 0.0, z=0.0)
    with pytest.raises(ValueError):
        L.grid_poses((1.0, 0.0), (0.0, 1.0), 1.0, z=0.0)


def test_drop_rule_on_stub_counts():
    counts = np.array([0, 5759, 5760, 5761, 57600])
    assert np.array_equal(L.keep_scans(counts, 64 * 900, 0.1), [False, False, True, True, True])   # FEWER than 10 % is dropped
    assert np.array_equal(L.keep_scans(counts, 64 * 900, 0.0), [True] * 5)
    assert L.render_chunk(64, 900, 4) == 233 and L.render_chunk(1, 1, 1) == 1024 and L.render_chunk(4096, 8192, 4) == 1


# ---- the export ---------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_additive():
    src = open(os.path.join(ROOT, "include", "ovn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ovn_render_scans\s*\(", code)
    assert re.search(r"#define\s+OVN_ABI_VERSION\s+11\b", code) and _lib.ABI_VERSION == 11
    assert "ovn_render_scans" in _lib.SIGNATURES          # (its types and arity against the header: tests/test_abi.py)
    _lib.build()
    lib = _lib.load()
    assert lib.ovn_abi_version() == 11 and hasattr(lib, "ovn_render_scans")
