"""CPU: the host side of the rolling TSDF window (overlapnet_amd/tsdf.py `RollingTsdfVolume`): `leaving_boxes`
against a brute-force set difference, the NumPy ring-storage model (tests/_tsdf_window_ref.py) against the dense statements on the
block at index_offset = base, the refusals that come before a GPU is touched, and the inputs of the GPU tests against their cap."""
import itertools

import numpy as np
import pytest

import _tsdf_ref as T
import _tsdf_window_ref as WR


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _NoGpu(object):
    """An engine stand-in that fails the test when a refusal comes too late."""
    @property
    def device(self):
        raise AssertionError("the GPU was touched before the arguments were checked")

    def __getattr__(self, name):
        raise AssertionError("engine.%s was reached before the arguments were checked" % name)


# ---- leaving_boxes -------------------------------------------------------------------------------------------------------------------
LATTICE = (16, 24, 16)
_STEPS = [(8, 0, 0), (-8, 0, 0), (0, 16, 0), (0, -16, 0), (0, 0, 8), (16, 0, 0), (-16, 0, 0), (8, -8, 0), (-16, 8, 0), (8, 8, 8),
          (-8, 16, -8), (8, -16, 8), (0, 0, 0), (16, 0, 0), (0, 24, 0), (0, 0, -16), (24, 8, 0), (8, 32, -8), (-40, -40, 40), (16, 24, 16)]


def _points(lo, hi):
    return set(itertools.product(range(lo[0], hi[0]), range(lo[1], hi[1]), range(lo[2], hi[2])))


@pytest.mark.parametrize("old", [(0, 0, 0), (-24, 8, -8)])
@pytest.mark.parametrize("step", _STEPS)
def test_leaving_boxes_are_the_set_difference(old, step):
    from overlapnet_amd import tsdf
    new = tuple(o + s for o, s in zip(old, step))
    top = tuple(o + n for o, n in zip(old, LATTICE))
    want = _points(old, top) - _points(new, tuple(b + n for b, n in zip(new, LATTICE)))
    boxes = tsdf.leaving_boxes(old, new, LATTICE)
    assert len(boxes) <= 3
    got = set()
    for lo, hi in boxes:
        assert all(o <= l < h <= t for o, l, h, t in zip(old, lo, hi, top)), "a box reaches outside the old window"
        pts = _points(lo, hi)
        assert pts and not (pts & got), "the boxes overlap or one is empty"
        got |= pts
    assert got == want
    if step == (0, 0, 0):
        assert boxes == []
    if any(abs(s) >= n for s, n in zip(step, LATTICE)):
        assert got == _points(old, top)


def test_follow_moves_by_multiples_of_shift_towards_the_sensor():
    from overlapnet_amd import tsdf
    vol = tsdf.RollingTsdfVolume.__new__(tsdf.RollingTsdfVolume)
    vol.nx, vol.ny, vol.nz, vol.voxel, vol.shift = 48, 32, 16, 0.5, 16
    vol.origin, vol.base = np.array([1.0, -2.0, 0.25]), (-24, -16, -8)
    at = lambda cell: vol.origin + (np.asarray(cell) + 0.5) * vol.voxel
    assert vol.cell_of(at((3, -7, 0))) == (3, -7, 0)
    assert vol.next_base(at((15, -15, 15))) == vol.base                     # less than `shift` from the centre (0, 0, 0)
    assert vol.next_base(at((16, -16, 0))) == (-8, -32, -8)
    assert vol.next_base(at((47, 0, -33))) == (8, -16, -40)                 # two shifts at once, towards zero
    with pytest.raises(ValueError):
        vol.cell_of((0.0, np.nan, 0.0))


# ---- the ring model against the dense statements ---------------------------------------------------------------------------------------
def test_ring_addressing_is_a_floor_modulus():
    for base, n in ((40, 72), (8, 24), (-32, 72), (-16, 24), (-8, 16), (0, 16), (-72, 72)):
        lat = WR.lattice_of_slots(base, n)
        assert sorted(lat.tolist()) == list(range(base, base + n))
        assert np.array_equal(WR.slots_of(lat, n), np.arange(n))
        assert all((int(i) - int(s)) % n == 0 for i, s in zip(lat, range(n)))
    g = np.random.default_rng(3)
    block = g.standard_normal((16, 24, 72)).astype(np.float32)
    for base in (WR.BASE, WR.BASE_NEG):
        ring = WR.to_ring(block, base)
        assert np.array_equal(WR.to_block(ring, base), block)
        # the same layout said another way: the block rolled by base mod n along every axis
        assert np.array_equal(ring, np.roll(block, tuple(b % n for b, n in zip(base[::-1], block.shape)), axis=(0, 1, 2)))


@pytest.mark.parametrize("base", [WR.BASE, WR.BASE_NEG])
def test_ring_integrate_is_the_statement_on_the_block(base):
    c = T.fused_case(WR.CASE)
    anchor = WR.anchor_for(base)
    g = np.random.default_rng(11)
    nz, ny, nx = WR.SHAPE[::-1]
    t0 = g.uniform(-1, 1, (nz, ny, nx)).astype(np.float32)            # not a fresh window: what was stored must be what is averaged
    w0 = g.integers(0, 3, (nz, ny, nx)).astype(np.float32)
    t, w = WR.integrate(WR.to_ring(t0, base), WR.to_ring(w0, base), anchor, base, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"], c["poses"])
    ref = T.integrate(t0, w0, anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"], c["poses"], index_offset=base)
    assert np.array_equal(_bits(WR.to_block(t, base)), _bits(ref["tsdf"])) and np.array_equal(_bits(WR.to_block(w, base)), _bits(ref["weight"]))
    assert ref["updated"].any()
    # and the block is the block of the dense volume with origin = anchor that holds it (a positive base only: a dense index is >= 0)
    if min(base) >= 0:
        dense = T.integrate(WR.in_dense(t0, base), WR.in_dense(w0, base), anchor, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"], c["poses"])
        cut = (slice(base[2], base[2] + nz), slice(base[1], base[1] + ny), slice(base[0], base[0] + nx))
        assert np.array_equal(_bits(dense["tsdf"][cut]), _bits(ref["tsdf"])) and np.array_equal(_bits(dense["weight"][cut]), _bits(ref["weight"]))


@pytest.mark.parametrize("base", [WR.BASE, WR.BASE_NEG])
def test_gpu_integrate_inputs_stay_within_the_ambiguity_cap(base):
    """What tests/test_gpu_tsdf_window.py compares with the statement: the float64 reference marks at most 5 % of the updated samples."""
    c = T.fused_case(WR.CASE)
    t0, w0 = T.fresh(WR.SHAPE)
    f64 = T.integrate(t0, w0, WR.anchor_for(base), T.VOXEL, T.TRUNC, T.MAX_WEIGHT, c["ranges"], c["poses"], dtype=np.float64, ambiguous=True,
                      index_offset=base)
    touched = f64["updated"].any(axis=0)
    share = (f64["ambiguous"] & touched).sum() / max(int(touched.sum()), 1)
    print("base %s: %d of %d samples updated, ambiguous share %.4f" % (base, touched.sum(), touched.size, share))
    assert touched.sum() > 1000 and share <= 0.05


def test_ring_shift_and_triangles_are_the_block_statements():
    base, shape = WR.BASE_NEG, WR.SHAPE
    d, w = WR.plane_block(shape, base, through=(4, -4, 0))
    anchor, voxel = np.array([1.0, -2.0, 0.5]), 0.25
    ring_d, ring_w = WR.to_ring(d, base), WR.to_ring(w, base)
    top = tuple(b + n - 1 for b, n in zip(base, shape))
    whole = WR.triangles(ring_d, ring_w, anchor, base, voxel, 1.0, base, top)
    assert whole.shape[0] > 500 and np.array_equal(_bits(whole), _bits(T.triangles(d, w, anchor, voxel, 1.0, index_offset=base)))
    lo, hi = (-2, -10, -6), (10, 2, 6)                                  # a box across the seam of every axis
    part = WR.triangles(ring_d, ring_w, anchor, base, voxel, 1.0, lo, hi)
    cut = (slice(lo[2] - base[2], hi[2] - base[2] + 1), slice(lo[1] - base[1], hi[1] - base[1] + 1), slice(lo[0] - base[0], hi[0] - base[0] + 1))
    assert part.shape[0] > 50 and np.array_equal(_bits(part), _bits(T.triangles(d[cut], w[cut], anchor, voxel, 1.0, index_offset=lo)))
    # shift: the samples of both windows keep slot and bits, every other slot is fresh, and the new window reads in lattice order
    for step in ((8, 0, 0), (-16, 8, 0), (0, 0, -8), (80, 0, 0), (0, -24, 0)):
        new = tuple(b + s for b, s in zip(base, step))
        t2, w2, fresh = WR.shift(ring_d, ring_w, base, new)
        blk_t, blk_w = WR.to_block(t2, new), WR.to_block(w2, new)
        k, j, i = np.meshgrid(*(np.arange(n) + b for n, b in zip(shape[::-1], new[::-1])), indexing="ij")
        old = (i >= base[0]) & (i <= top[0]) & (j >= base[1]) & (j <= top[1]) & (k >= base[2]) & (k <= top[2])
        assert np.all(blk_t[~old] == 1) and np.all(blk_w[~old] == 0) and fresh.sum() == (~old).sum()
        sel = (k[old] - base[2], j[old] - base[1], i[old] - base[0])
        assert np.array_equal(_bits(blk_t[old]), _bits(d[sel])) and np.array_equal(_bits(blk_w[old]), _bits(w[sel]))
        assert np.array_equal(_bits(t2[~fresh]), _bits(ring_d[~fresh]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_the_gpu():
    from overlapnet_amd import odometry, tsdf
    ok = (72, 24, 16)
    tsdf.check_window(ok, (40, 8, 8))
    tsdf.check_window(ok, (-(1 << 20), 0, (1 << 20) - 16))
    for shape, base in (((70, 24, 16), (0, 0, 0)), ((72, 24, 8), (0, 0, 0)), ((72, 20, 16), (0, 0, 0)),      # not a multiple of 8, < 16
                        (ok, (4, 0, 0)), (ok, (0, -12, 0)),                                                    # base not a multiple of 8
                        (ok, ((1 << 20) - 64, 0, 0)), (ok, (0, -(1 << 20) - 8, 0)), (ok, (0, 0, 1 << 20)),     # |I| > 2^20
                        ((2048, 2048, 1024), (0, 0, 0))):                                                      # over 2^31 - 1 samples
        with pytest.raises(ValueError):
            tsdf.check_window(shape, base)
    assert tsdf.window_shape((14.3, 4.8, 1.0), 0.2) == (72, 24, 16) and tsdf.window_shape(48.0, 0.2) == (240, 240, 240)
    for kw in (dict(extent=(10, 10), voxel=0.2), dict(extent=(10, 0, 10), voxel=0.2), dict(extent=10, voxel=0.0),
               dict(extent=10, voxel=0.2, shift=4), dict(extent=10, voxel=0.2, shift=12), dict(extent=10, voxel=0.2, trunc=0.0),
               dict(extent=10, voxel=0.2, anchor=(0, np.inf, 0)), dict(extent=(4000, 4000, 400), voxel=0.1)):
        with pytest.raises(ValueError):
            tsdf.RollingTsdfVolume(_NoGpu(), **kw)
    # a triangle box that reaches outside the window, and a move past the lattice
    vol = tsdf.RollingTsdfVolume.__new__(tsdf.RollingTsdfVolume)
    vol.engine, vol.voxel, vol.n_scans, vol.shift = _NoGpu(), 0.2, 0, 8
    vol.nx, vol.ny, vol.nz = ok
    vol.base, vol.origin = (40, 8, 8), np.zeros(3)
    for box in (((39, 8, 8), (50, 10, 10)), ((40, 8, 8), (112, 10, 10)), ((40, 8, 8), (50, 10, 24)), ((50, 8, 8), (49, 10, 10))):
        with pytest.raises(ValueError):
            vol.triangles(box=box)
    with pytest.raises(ValueError):
        vol.triangles(min_weight=float("nan"))
    with pytest.raises(ValueError):
        vol.follow(((1 << 20) * 0.2, 0.0, 0.0))
    # the following tracker: a window a scan can reach past
    sensor = dict(proj_h=16, proj_w=90, max_range=20.0)
    for kw in (dict(extent=(40.0, 48.0, 8.0), voxel=0.2), dict(extent=(48.0, 44.0, 8.0), voxel=0.2),
               dict(extent=(46.0, 46.0, 8.0), voxel=0.2, shift=16), dict(extent=(48.0, 48.0, 8.0), voxel=0.2, trunc=3.0)):
        with pytest.raises(ValueError, match="max_range"):
            odometry.RollingTsdfOdometry(_NoGpu(), **kw, **sensor)
    with pytest.raises(ValueError):
        odometry.RollingTsdfOdometry(_NoGpu(), (48.0, 48.0, 8.0), 0.2, tolerance=3, **sensor)
    with pytest.raises(AssertionError, match="GPU was touched"):       # 24 m >= 20 + 0.8 + 0.2 + 1.6: this one is accepted
        odometry.RollingTsdfOdometry(_NoGpu(), (48.0, 48.0, 8.0), 0.2, **sensor)
    with pytest.raises(ValueError):
        odometry.estimate_poses(_NoGpu(), np.zeros((10, 4), np.float32), [0, 10], window=30.0, max_range=20.0)
