"""NumPy model of the rolling TSDF window's storage (include/ovn_hip.h "A TSDF volume that follows the sensor"):
integrate, shift and triangles on RING storage.

The float32 statements are those of tests/_tsdf_ref.py, taken on the block at `index_offset = base` (the helper takes a negative offset
as it stands: an index only ever enters as np.arange(n) + i0).  What this file states is the addressing: sample I of an axis lives in
slot I mod n, floor modulus, so slot s holds lattice index base + ((s - base) mod n).  Plus the cases the host and the GPU tests share.
"""
import numpy as np

import _tsdf_ref as T

F32 = np.float32

SHAPE, BASE = (72, 24, 16), (40, 8, 8)          # nx no multiple of 64; the seam inside a 64-lane run on x, inside the volume on y and z
BASE_NEG = (-32, -16, -8)
DENSE = (112, 32, 24)                           # the dense volume with origin = anchor that contains SHAPE at BASE
CASE = "33x17x9"                                # the scans and poses of T.fused_case


def lattice_of_slots(base, n):
    """(n) int64: the lattice index that lives in each slot of an axis."""
    s = np.arange(n, dtype=np.int64)
    return int(base) + np.mod(s - int(base), n)


def slots_of(index, n):
    """The slot of lattice indices: floor modulus (np.mod is one)."""
    return np.mod(np.asarray(index, np.int64), n)


def _gather(storage, base, lo, hi):
    """The samples lo <= (I, J, K) < hi of a window in lattice order, (hi - lo)[::-1] shaped."""
    nz, ny, nx = storage.shape
    ix = [slots_of(np.arange(lo[a], hi[a]), n) for a, n in enumerate((nx, ny, nz))]
    for a, n in enumerate((nx, ny, nz)):
        assert base[a] <= lo[a] <= hi[a] <= base[a] + n, "samples outside the window"
    return storage[np.ix_(ix[2], ix[1], ix[0])]


def to_block(storage, base):
    """The whole window in lattice order: block[k, j, i] = sample base + (i, j, k)."""
    nz, ny, nx = storage.shape
    return _gather(storage, base, base, (base[0] + nx, base[1] + ny, base[2] + nz))


def to_ring(block, base):
    """The inverse of to_block: the block in lattice order laid into ring storage."""
    nz, ny, nx = block.shape
    out = np.empty_like(block)
    ix = [slots_of(np.arange(base[a], base[a] + n), n) for a, n in enumerate((nx, ny, nz))]
    out[np.ix_(ix[2], ix[1], ix[0])] = block
    return out


def integrate(tsdf, weight, anchor, base, voxel, trunc, max_weight, ranges, poses, **kw):
    """ovn_tsdf_window_integrate on ring storage -> (tsdf, weight) in ring storage.  **kw: those of T.integrate."""
    o = T.integrate(to_block(tsdf, base), to_block(weight, base), anchor, voxel, trunc, max_weight, ranges, poses, index_offset=base, **kw)
    return to_ring(o["tsdf"].astype(F32), base), to_ring(o["weight"].astype(F32), base)


def shift(tsdf, weight, old_base, new_base):
    """ovn_tsdf_window_shift: every slot whose sample under new_base was not in the old window becomes (1, 0) -> (tsdf, weight, the
    (nz,ny,nx) bool mask of those slots)."""
    nz, ny, nx = tsdf.shape
    stays = []
    for a, n in enumerate((nx, ny, nz)):
        new = lattice_of_slots(new_base[a], n)
        stays.append((new >= old_base[a]) & (new < old_base[a] + n))
    fresh = ~(stays[2][:, None, None] & stays[1][None, :, None] & stays[0][None, None, :])
    return np.where(fresh, F32(1), tsdf), np.where(fresh, F32(0), weight), fresh


def triangles(tsdf, weight, anchor, base, voxel, min_weight, box_lo, box_hi):
    """ovn_tsdf_window_triangles: the cells whose low corner lies in box_lo <= (I, J, K) < box_hi, in ascending cell order within the box."""
    hi = tuple(int(v) + 1 for v in box_hi)                  # the samples of those cells
    if any(h - l < 2 for l, h in zip(box_lo, hi)):
        return np.zeros((0, 3, 3), F32)
    return T.triangles(_gather(tsdf, base, box_lo, hi), _gather(weight, base, box_lo, hi), anchor, voxel, min_weight, index_offset=box_lo)


def anchor_for(base):
    """The anchor that puts sample `base` of the lattice where the fused case's volume starts: the window then holds the case's scene."""
    return T._origins()[CASE] - np.asarray(base, np.float64) * T.VOXEL


def plane_block(shape, base, through, normal=(0.37, -0.61, 0.70)):
    """(tsdf, weight) in lattice order for the window `shape` at `base`: the signed distance, in voxels, to the plane through lattice
    point `through`; weight 1 but for the aligned brick at base + (8, 0, 0), which nobody has seen."""
    nx, ny, nz = shape
    nrm = np.asarray(normal) / np.linalg.norm(normal)
    k, j, i = np.meshgrid(np.arange(nz) + base[2], np.arange(ny) + base[1], np.arange(nx) + base[0], indexing="ij")
    d = (i - through[0]) * nrm[0] + (j - through[1]) * nrm[1] + (k - through[2]) * nrm[2]
    w = np.ones((nz, ny, nx), F32)
    w[0:8, 0:8, 8:16] = 0
    return d.astype(F32), w


def in_dense(block, base, dense_shape=DENSE):
    """The block (lattice order) laid into a dense (nz,ny,nx) array of zeros at sample `base`: as weights, a dense volume with origin =
    anchor that has seen the window's samples and nothing else."""
    nx, ny, nz = dense_shape
    out = np.zeros((nz, ny, nx), block.dtype)
    bz, by, bx = block.shape
    out[base[2]:base[2] + bz, base[1]:base[1] + by, base[0]:base[0] + bx] = block
    return out
