"""Triangle meshes for `ovn_render_scans`: validation, PLY / OBJ readers, a PLY writer, the ray tables of a sensor and the bounding-volume hierarchy.

The hierarchy is built on the host, once per mesh, in vectorised NumPy (no Python loop over triangles; one step per tree LEVEL):
triangles sorted by the 30-bit Morton code of their centroid, leaves of 4 consecutive triangles, an implicit complete binary tree over
the leaves (root 1, children 2i and 2i + 1, leaves NL .. 2 NL - 1, NL a power of two), boxes reduced bottom-up and padded outwards.
The layout and the padding are the contract of include/ovn_hip.h and DESIGN.md section 28.
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Tuple

import numpy as np

MAX_TRIANGLES = 1 << 27          # OVN_RENDER_MAX_TRIANGLES
LEAF_TRIANGLES = 4               # OVN_RENDER_LEAF_TRIANGLES
BOX_PAD_REL = 2.0 ** -12         # every box grows by this fraction of the mesh's scale on each side


def direction_tables(proj_H: int, proj_W: int, fov_up: float, fov_down: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """cos / sin of the azimuth of every column and of the pitch of every row, evaluated in float64 and rounded to float32: the ray
    through the centre of the pixel `range_projection` would put a point into.  Returns (cos_az (W), sin_az (W), cos_pitch (H),
    sin_pitch (H))."""
    h, w = int(proj_H), int(proj_W)
    up = float(fov_up) / 180.0 * np.pi
    down = float(fov_down) / 180.0 * np.pi
    fov = abs(down) + abs(up)
    az = -(((np.arange(w, dtype=np.float64) + 0.5) / w) * 2.0 - 1.0) * np.pi
    pitch = (1.0 - (np.arange(h, dtype=np.float64) + 0.5) / h) * fov - abs(down)
    return (np.cos(az).astype(np.float32), np.sin(az).astype(np.float32), np.cos(pitch).astype(np.float32),
            np.sin(pitch).astype(np.float32))


def _spread3(v: np.ndarray) -> np.ndarray:
    """The 10 low bits of v, two zero bits between neighbours."""
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton30(points: np.ndarray) -> np.ndarray:
    """30-bit Morton code of every row of (N,3) points inside their common bounding box (an axis of zero extent codes 0)."""
    p = np.asarray(points, np.float64)
    lo = p.min(axis=0)
    ext = p.max(axis=0) - lo
    scale = np.where(ext > 0, 1023.0 / np.where(ext > 0, ext, 1.0), 0.0)
    g = np.clip(np.floor((p - lo) * scale), 0, 1023).astype(np.uint32)
    return (_spread3(g[:, 0]) << np.uint32(2)) | (_spread3(g[:, 1]) << np.uint32(1)) | _spread3(g[:, 2])


def box_padding(vertices: np.ndarray) -> float:
    """The outward padding of every box: BOX_PAD_REL times the larger of the mesh's extent and its largest |coordinate|."""
    v = np.asarray(vertices, np.float64)
    scale = max(float((v.max(axis=0) - v.min(axis=0)).max()), float(np.abs(v).max()))
    return BOX_PAD_REL * scale


def build_bvh(vertices: np.ndarray, triangles: np.ndarray) -> Tuple[np.ndarray, np.ndarray, int]:
    """(nodes (2 NL, 8) float32, order (T) int32, NL).  Row i of `nodes` is lo.x lo.y lo.z 0 hi.x hi.y hi.z 0 of node i; row 0 is
    unused; an empty node (a leaf past the last triangle, or an inner node over such leaves only) has lo = +inf, hi = -inf."""
    v = np.asarray(vertices, np.float32)
    tri = np.asarray(triangles, np.int64)
    t = tri.shape[0]
    corners = v[tri]                                          # (T,3,3)
    order = np.argsort(morton30(corners.astype(np.float64).mean(axis=1)), kind="stable").astype(np.int32)
    leaves = -(-t // LEAF_TRIANGLES)
    nl = 1
    while nl < leaves:
        nl *= 2
    sorted_corners = corners[order]
    lo = np.full((nl * LEAF_TRIANGLES, 3), np.inf, np.float32)
    hi = np.full((nl * LEAF_TRIANGLES, 3), -np.inf, np.float32)
    lo[:t] = sorted_corners.min(axis=1)                       # exact: a minimum of float32 values
    hi[:t] = sorted_corners.max(axis=1)
    lo = lo.reshape(nl, LEAF_TRIANGLES, 3).min(axis=1)
    hi = hi.reshape(nl, LEAF_TRIANGLES, 3).max(axis=1)
    nodes = np.zeros((2 * nl, 8), np.float32)
    m = nl
    while True:                                               # one step per level: nodes m .. 2m - 1
        nodes[m:2 * m, 0:3] = lo
        nodes[m:2 * m, 4:7] = hi
        if m == 1:
            break
        lo = np.minimum(lo[0::2], lo[1::2])
        hi = np.maximum(hi[0::2], hi[1::2])
        m //= 2
    pad = np.float32(box_padding(v))
    # the float32 subtraction may round towards the box: one more step outwards makes the padding at least `pad`
    nodes[1:, 0:3] = np.nextafter(nodes[1:, 0:3] - pad, np.float32(-np.inf))
    nodes[1:, 4:7] = np.nextafter(nodes[1:, 4:7] + pad, np.float32(np.inf))
    nodes[0, 0:3], nodes[0, 4:7] = np.inf, -np.inf
    return nodes, order, nl


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


class TriangleMesh(object):
    """vertices (V,3) float32 and triangles (T,3) int32, validated: finite vertices, 1 <= T <= 2^27, every index in [0, V)."""

    def __init__(self, vertices, triangles):
        v = np.asarray(vertices)
        f = np.asarray(triangles)
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
            raise ValueError("vertices must be (V,3) with V >= 1, got shape %s" % (v.shape,))
        if v.dtype.kind != "f":
            raise ValueError("vertices must be floating point, got %s" % v.dtype)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError("triangles must be (T,3), got shape %s" % (f.shape,))
        if f.dtype.kind not in "iu":
            raise ValueError("triangles must be integers, got %s" % f.dtype)
        if not 1 <= f.shape[0] <= MAX_TRIANGLES:
            raise ValueError("%d triangles outside 1 .. 2^27" % f.shape[0])
        v32 = np.ascontiguousarray(v, np.float32)
        if not np.isfinite(v32).all():
            raise ValueError("vertices must be finite in float32 (%d are not)" % int((~np.isfinite(v32)).any(axis=1).sum()))
        if v.shape[0] > 2 ** 31 - 1:
            raise ValueError("%d vertices exceed 2^31 - 1" % v.shape[0])
        if int(f.min()) < 0 or int(f.max()) >= v.shape[0]:
            raise ValueError("triangle indices span %d .. %d, outside the %d vertices" % (int(f.min()), int(f.max()), v.shape[0]))
        self.vertices = v32
        self.triangles = np.ascontiguousarray(f, np.int32)
        self._bvh = None
        self._device: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()

    @property
    def n_vertices(self) -> int:
        return self.vertices.shape[0]

    @property
    def n_triangles(self) -> int:
        return self.triangles.shape[0]

    @property
    def bvh(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """(nodes, order, leaves) of `build_bvh`, built on first use."""
        if self._bvh is None:
            self._bvh = build_bvh(self.vertices, self.triangles)
        return self._bvh

    def device(self, engine, with_bvh: bool = True) -> Dict[str, object]:
        """The device copies for `engine` (made once per engine): vertices, triangles and, when asked for, nodes / order / leaves."""
        import torch
        d = self._device.get(engine)
        if d is None:
            d = {"vertices": torch.from_numpy(self.vertices).to(engine.device),
                 "triangles": torch.from_numpy(self.triangles).to(engine.device)}
            self._device[engine] = d
        if with_bvh and "nodes" not in d:
            nodes, order, nl = self.bvh
            d["nodes"] = torch.from_numpy(nodes).to(engine.device)
            d["order"] = torch.from_numpy(order).to(engine.device)
            d["leaves"] = nl
        return d

    # -- readers ------------------------------------------------------------------------------------
    @classmethod
    def from_ply(cls, path: str) -> "TriangleMesh":
        """ASCII or binary_little_endian PLY with a `vertex` element that has x, y, z and a `face` element whose one list property
        (`vertex_indices` or `vertex_index`) holds triangles.  Anything else raises ValueError naming what was found."""
        with open(path, "rb") as fh:
            data = fh.read()
        if not data.startswith(b"ply"):
            raise ValueError("%s: not a PLY file (starts with %r)" % (path, data[:8]))
        end = data.find(b"end_header")
        if end < 0:
            raise ValueError("%s: PLY header has no end_header" % path)
        nl = data.find(b"\n", end)
        if nl < 0:
            raise ValueError("%s: PLY header is not terminated" % path)
        lines = [ln.strip() for ln in data[:end].decode("ascii", "replace").splitlines()]
        body = data[nl + 1:]
        fmt = None
        elements = []          # [name, count, [property tuples]]
        for ln in lines[1:]:
            tok = ln.split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = " ".join(tok[1:])
            elif tok[0] == "element" and len(tok) == 3:
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property" and elements:
                if tok[1] == "list" and len(tok) == 5:
                    elements[-1][2].append(("list", tok[2], tok[3], tok[4]))
                elif len(tok) == 3:
                    elements[-1][2].append(("scalar", tok[1], tok[2]))
                else:
                    raise ValueError("%s: cannot parse PLY header line %r" % (path, ln))
            else:
                raise ValueError("%s: cannot parse PLY header line %r" % (path, ln))
        if fmt not in ("ascii 1.0", "binary_little_endian 1.0"):
            raise ValueError("%s: PLY format %r; ascii 1.0 and binary_little_endian 1.0 are read" % (path, fmt))
        names = [e[0] for e in elements]
        if names != ["vertex", "face"]:
            raise ValueError("%s: PLY elements %s; expected vertex then face" % (path, names))
        (_, nv, vprops), (_, nf, fprops) = elements
        for p in vprops:
            if p[0] != "scalar" or p[1] not in _PLY_TYPES:
                raise ValueError("%s: vertex property %s is not a scalar of a known type" % (path, " ".join(p)))
        vnames = [p[2] for p in vprops]
        if any(c not in vnames for c in "xyz"):
            raise ValueError("%s: vertex properties %s lack x, y or z" % (path, vnames))
        if (len(fprops) != 1 or fprops[0][0] != "list" or fprops[0][3] not in ("vertex_indices", "vertex_index")
                or fprops[0][1] not in _PLY_TYPES or fprops[0][2] not in _PLY_TYPES
                or _PLY_TYPES[fprops[0][1]][0] == "f" or _PLY_TYPES[fprops[0][2]][0] == "f"):
            raise ValueError("%s: face properties %s; expected one integer list vertex_indices"
                             % (path, [" ".join(p) for p in fprops]))
        if fmt.startswith("ascii"):
            tok = body.split()
            nvt = nv * len(vprops)
            if len(tok) < nvt + 4 * nf:
                raise ValueError("%s: %d values for %d vertices and %d triangular faces" % (path, len(tok), nv, nf))
            try:
                vt = np.array(tok[:nvt], dtype=np.float64).reshape(nv, len(vprops))
                ft = np.array(tok[nvt:nvt + 4 * nf], dtype=np.float64).reshape(nf, 4) if nf else np.zeros((0, 4))
            except ValueError as e:
                raise ValueError("%s: a value of the PLY body is not a number (%s)" % (path, e))
            counts = ft[:, 0]
            if nf and not (counts == 3).all():
                raise ValueError("%s: a face with %d vertices; only triangles are read" % (path, int(counts[counts != 3][0])))
            if len(tok) != nvt + 4 * nf:
                raise ValueError("%s: %d values after the last face" % (path, len(tok) - nvt - 4 * nf))
            xyz = np.stack([vt[:, vnames.index(c)] for c in "xyz"], axis=1)
            faces = ft[:, 1:].astype(np.int64)
        else:
            vdt = np.dtype([(p[2], "<" + _PLY_TYPES[p[1]]) for p in vprops])
            fdt = np.dtype([("n", "<" + _PLY_TYPES[fprops[0][1]]), ("i", "<" + _PLY_TYPES[fprops[0][2]], (3,))])
            if len(body) < nv * vdt.itemsize:
                raise ValueError("%s: %d body bytes, %d vertices need %d" % (path, len(body), nv, nv * vdt.itemsize))
            vt = np.frombuffer(body, vdt, nv)
            rest = body[nv * vdt.itemsize:]
            # read as triangles as far as the bytes go: the first record whose count is not 3 is where a polygon starts
            head = np.frombuffer(rest, fdt, min(nf, len(rest) // fdt.itemsize))["n"]
            if (head != 3).any():
                raise ValueError("%s: a face with %d vertices; only triangles are read" % (path, int(head[head != 3][0])))
            if len(rest) != nf * fdt.itemsize:
                raise ValueError("%s: %d bytes of faces, %d triangular faces need %d (truncated, or a face is no triangle)"
                                 % (path, len(rest), nf, nf * fdt.itemsize))
            ft = np.frombuffer(rest, fdt, nf)
            if nf and not (ft["n"] == 3).all():
                raise ValueError("%s: a face with %d vertices; only triangles are read" % (path, int(ft["n"][ft["n"] != 3][0])))
            xyz = np.stack([vt[c].astype(np.float64) for c in "xyz"], axis=1)
            faces = ft["i"].astype(np.int64)
        return cls(xyz.astype(np.float32), faces)

    def to_ply(self, path: str) -> None:
        """binary_little_endian PLY: float x, y, z per vertex and a `uchar int vertex_indices` list per face.  `from_ply` reads it
        back to the same arrays."""
        head = ("ply\nformat binary_little_endian 1.0\ncomment overlapnet_amd TriangleMesh\nelement vertex %d\nproperty float x\n"
                "property float y\nproperty float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                % (self.n_vertices, self.n_triangles))
        faces = np.empty(self.n_triangles, np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        faces["n"] = 3
        faces["i"] = self.triangles
        with open(path, "wb") as fh:
            fh.write(head.encode("ascii"))
            fh.write(self.vertices.astype("<f4").tobytes())
            fh.write(faces.tobytes())

    @classmethod
    def from_obj(cls, path: str) -> "TriangleMesh":
        """Wavefront OBJ: `v x y z` and triangular `f a b c` lines (a/b/c forms take the part before the first slash; negative
        indices count from the end); every other line is ignored.  A face that is no triangle raises."""
        verts, faces = [], []
        with open(path, "r") as fh:
            for ln in fh:
                tok = ln.split()
                if not tok:
                    continue
                if tok[0] == "v":
                    verts.append([float(x) for x in tok[1:4]])
                elif tok[0] == "f":
                    if len(tok) != 4:
                        raise ValueError("%s: a face with %d vertices; only triangles are read" % (path, len(tok) - 1))
                    ids = [int(x.split("/")[0]) for x in tok[1:]]
                    faces.append([i - 1 if i > 0 else len(verts) + i for i in ids])
        return cls(np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3))
