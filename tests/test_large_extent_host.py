"""CPU: the arithmetic of tests/test_gpu_large_extent.py -- that every case of tests/_large_extent.py really carries its buffer past
the boundary it claims, that a real item straddles each boundary, and that a truncated offset of a real item lands where checks
(b) / (c) of the GPU test see it -- plus the refusals that need no GPU, the checks' own power on small host tensors, and the offset
argument added to tests/_mcl_ref.py's lookup."""
import numpy as np
import pytest
import torch

import _large_extent as LX
import _mcl_ref as MR

CASE_IDS = [c.name for c in LX.CASES]


@pytest.mark.parametrize("case", LX.CASES, ids=CASE_IDS)
def test_case_crosses_what_it_claims(case):
    total = case.n * case.per_item
    if case.cap is None:
        assert total - 1 >= LX.B31                                    # the largest index passes 2^31 elements
        assert LX.B31 in case.crosses
    else:
        assert total <= case.cap < LX.B31 + 1                        # the header caps the elements: only the byte offset can cross
        assert (total - 1) * case.elem_bytes >= LX.B32 and case.crosses == (LX.B30,) and case.elem_bytes == 4
    assert total * case.elem_bytes <= 40e9                            # one buffer of a case alone stays far below the 40 GB of a test
    reals = LX.real_items(case)
    assert reals[0] == 0 and reals[-1] == case.n - 1 and len(set(reals)) == len(reals)
    for b in case.crosses:
        s = LX.straddler(case.per_item, b)
        lo, hi = LX.extent(case, s)
        assert s in reals and s + 1 in reals and lo <= b < hi         # the item that holds element b, and the one after it
        if case.per_item > 1 and b % case.per_item:
            assert lo < b < hi                                        # it straddles: it starts before the boundary
        if case.elem_bytes == 4:
            assert (b * case.elem_bytes) % LX.B32 == 0                # 2^30 and 2^31 elements are byte offsets 2^32 and 2^33
    assert len(reals) < 16 and reals[1] > 1                           # almost everything is empty


@pytest.mark.parametrize("case", LX.CASES, ids=CASE_IDS)
def test_truncated_offsets_of_real_items_are_seen(case):
    """A 32-bit index (mod 2^32, or that as a signed integer), in elements or in bytes, of a real item's first or last element: it
    never lands in the item's own extent -- so the item keeps its sentinel (check c / b), and the write shows up in another real
    item (b), in an empty one (c), or in front of the buffer (a guard, or a fault).  Every real item past a boundary has such a
    truncation; item 0 has only the signed-byte one at most."""
    past = 0
    for item in LX.real_items(case):
        hits = LX.truncated_targets(case, item)
        assert all(h != "own" for _, _, h in hits), (case.name, item, hits)
        lo, hi = LX.extent(case, item)
        if (hi - 1) * case.elem_bytes >= LX.B32:
            assert any(kind == "byte" for kind, _, _ in hits), (case.name, item)
            past += 1
        if hi - 1 >= LX.B31:
            assert any(kind == "element" for kind, _, _ in hits), (case.name, item)
    assert past >= 2                                                  # at least the straddler's successor and the last item


def test_truncations():
    assert LX.truncations(5) == [] and LX.truncations(LX.B31 - 1) == []
    assert LX.truncations(LX.B31) == [-LX.B31] and LX.truncations(LX.B31 + 7) == [7 - LX.B31]
    assert LX.truncations(LX.B32 + 3) == [3] and LX.truncations(LX.B32 + LX.B31) == [-LX.B31, LX.B31]


def test_guarded_checks_see_a_stray_write_a_wrong_item_and_a_left_sentinel():
    n, per = 9, 5
    reals = [0, 4, 8]
    small = torch.arange(15, dtype=torch.float32).reshape(3, 5)
    sb = small.view(torch.int32)
    m1 = LX.f32_bits(-1.0)

    def fresh():
        g = LX.Guarded((n, per), torch.float32, "cpu")
        assert g.count_sentinel() == n * per and g.guards_intact() and bool(torch.isnan(g.t).all())
        g.t.fill_(-1.0)
        g.t[reals] = small
        return g

    g = fresh()
    assert LX.check_items(g, per, n, reals, sb, m1) == {"guards": True, "real_diff": 0, "empty_diff": 0, "sentinel_left": 0}
    g.t[3, 2] = 7.0                                                                     # a stray write in bounds
    assert LX.check_items(g, per, n, reals, sb, m1)["empty_diff"] == 1
    g = fresh()
    g.t[4, 0] = -0.0 + 5.0 + 1e-6                                                       # a real item a little off
    assert LX.check_items(g, per, n, reals, sb, m1)["real_diff"] == 1
    g = fresh()
    g.bits[7 * per + 1] = LX.SENTINEL_F32_BITS                                          # an element nobody wrote
    r = LX.check_items(g, per, n, reals, sb, m1)
    assert r["sentinel_left"] == 1 and r["empty_diff"] == 1
    g = fresh()
    g.raw[g.front.numel() - 1] = 0                                                      # one word in front of the output
    assert not g.guards_intact()
    g = fresh()
    g.raw[g.front.numel() + g.numel] = 0                                                # one word behind it
    assert not LX.check_items(g, per, n, reals, sb, m1)["guards"]
    gi = LX.Guarded((6,), torch.int32, "cpu")
    assert int(gi.t[0]) == LX.SENTINEL_I32 and gi.bytes == 2 * LX.GUARD_BYTES + 24
    # a row as the empty value (the leg: the feature volume of an all -1 image)
    g = fresh()
    g.t[:] = small[1]
    g.t[reals] = small
    assert LX.check_items(g, per, n, reals, sb, sb[1])["empty_diff"] == 0
    assert LX.check_items(g, per, n, reals, sb, sb[2])["empty_diff"] == 6 * per


def test_size_refusals_need_no_gpu():
    """The limits the projection and ground-truth kernels assume, refused with OVN_ERR_ARG before anything else is looked at (no
    context, no buffer, no launch): H*W <= 2^31 - 1, at most 65535 scans per ovn_project call, at most 2^31 - 2 per
    ovn_gt_overlap_counts call.  One step inside each limit the call gets as far as its NULL context."""
    from overlapnet_amd import _lib
    lib = _lib.load()
    N = None
    big, ok = (46341, 46341), (46340, 46341)                           # 2^31 + 4 633 resp. 2^31 - 41 708 pixels
    assert big[0] * big[1] > LX.B31 - 1 >= ok[0] * ok[1]

    def project(n_scans, h, w):
        return lib.ovn_project(N, N, N, n_scans, 0, h, w, 3.0, -25.0, 50.0, N, N, N, N, N, N, 1, 1, 0, N)

    def semantic(n_scans, h, w):
        return lib.ovn_project_semantic(N, N, N, n_scans, 0, h, w, 3.0, -25.0, 50.0, N, 20, N, N, N, N, N, N, N, N, 1, 1, 0, 0, N)

    calls = {
        "ovn_project": lambda h, w: project(1, h, w),
        "ovn_project_semantic": lambda h, w: semantic(1, h, w),
        "ovn_projection_angles": lambda h, w: lib.ovn_projection_angles(N, N, 1, h, w, 3.0, -25.0, 50.0, N, N, N, N),
        "ovn_normals": lambda h, w: lib.ovn_normals(N, N, N, 1, h, w, N, N),
        "ovn_gt_range_images": lambda h, w: lib.ovn_gt_range_images(N, N, N, 1, 0, N, N, h, w, 3.0, -25.0, 50.0, N, N),
        "ovn_gt_overlap_counts": lambda h, w: lib.ovn_gt_overlap_counts(N, N, N, 1, h, w, N, N),
    }
    for name, call in calls.items():
        assert call(*big) == 1, name
        msg = lib.ovn_last_error()
        assert name.encode() + b":" in msg and b"2^31 - 1" in msg and b"46341 x 46341" in msg, msg
        assert call(*ok) == 1 and b"ctx is NULL" in lib.ovn_last_error(), name
        assert call(65536, 65536) == 1 and b"2^31 - 1" in lib.ovn_last_error(), name      # 2^32 pixels: H * W wraps to 0 in 32 bits

    assert project(65536, 64, 900) == 1 and b"at most 65535" in lib.ovn_last_error()
    assert project(65535, 64, 900) == 1 and b"ctx is NULL" in lib.ovn_last_error()
    assert lib.ovn_gt_overlap_counts(N, N, N, 2 ** 31 - 1, 64, 900, N, N) == 1 and b"2^31 - 2" in lib.ovn_last_error()
    assert lib.ovn_gt_overlap_counts(N, N, N, 2 ** 31 - 2, 64, 900, N, N) == 1 and b"ctx is NULL" in lib.ovn_last_error()
    assert lib.ovn_abi_version() == _lib.ABI_VERSION                # refusals of inputs that never worked: the ABI stays


def test_mcl_lookup_cell_offset_is_the_statement_on_a_block():
    rs = np.random.default_rng(3)
    nx, ny, M = 23, 17, 9
    table = rs.integers(-1, M + 2, nx * ny).astype(np.int32)
    x = rs.uniform(-2, nx + 2, 400).astype(np.float32)
    y = rs.uniform(-2, ny + 2, 400).astype(np.float32)
    want = MR.lookup(x, y, table, 0.0, 0.0, 1.0, nx, ny, M)
    assert np.array_equal(MR.lookup(x, y, table, 0.0, 0.0, 1.0, nx, ny, M, cell_offset=0), want)      # offset 0: the statement
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 50
    r0, nr = 11, 4                                                     # rows 11..14 alone, given as a block
    rows = np.floor(y).astype(np.int64)
    sel = (rows >= r0) & (rows < r0 + nr)
    assert sel.sum() > 40
    got = MR.lookup(x[sel], y[sel], table[r0 * nx:(r0 + nr) * nx], 0.0, 0.0, 1.0, nx, ny, M, cell_offset=r0 * nx)
    assert np.array_equal(got, want[sel])
    with pytest.raises(IndexError):                                    # a position whose cell the block does not hold
        MR.lookup(x, y, table[r0 * nx:(r0 + nr) * nx], 0.0, 0.0, 1.0, nx, ny, M, cell_offset=r0 * nx)


def test_leg_train_activations_cross_where_the_case_says():
    """Layer-major activations of the reference leg at n = LEG_TRAIN_N: the buffer passes 2^31 elements, a layer block starts past
    byte offset 2^32, and the last scan block's feature volumes (the last layer block) lie past 2^31 elements."""
    from tools import synthetic as S
    act = LX.leg_activation_sizes(64, 900, 4, S.REFERENCE_MODEL_CFG)
    n, sb = LX.LEG_TRAIN_N, LX.LEG_TRAIN_BLOCK
    total = sum(act)
    assert total == 951776 and act[-1] == 360 * 128 and n % sb == 0
    smallest = -(-LX.B31 // total)                                    # 2257 scans; n is the next multiple of the scan block
    assert (smallest - 1) * total < LX.B31 <= smallest * total and smallest <= n < smallest + sb
    assert n * total * 4 <= 40e9
    starts = [n * sum(act[:li]) for li in range(len(act))]
    assert any(s_ * 4 >= LX.B32 for s_ in starts)
    first_real_of_last_block = starts[-1] + (n - sb) * act[-1]
    assert first_real_of_last_block >= LX.B31
    for off in (first_real_of_last_block, starts[-1] + n * act[-1] - 1):
        assert LX.truncations(off) and all(t < starts[-1] + (n - sb) * act[-1] for t in LX.truncations(off))


def test_project_dummy_scan_puts_the_real_points_past_2_31():
    d = LX.PROJECT_DUMMY_POINTS
    assert (d - 1) * 4 + 3 < LX.B31 + 4 * 130000 and d * 4 >= LX.B31 and d < LX.B32      # x of the first real point: element 2^31 + 516 352
    assert all(t < 0 for t in LX.truncations(d * 4)) and (d + 124668) * 4 * 4 <= 9e9     # a signed 32-bit offset reads in front of `points`


def test_tsdf_and_raycast_statements_take_a_block_of_a_larger_volume():
    """index_offset of tests/_tsdf_ref.py (integrate, triangles) and tests/_raycast_ref.py (raycast): at (0, 0, 0) the statement itself,
    and on a block of a small volume the bits of the whole volume's statement there."""
    import _raycast_ref as RC
    import _tsdf_ref as T
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
    shape, origin = (12, 10, 16), (-1.3, 0.4, -2.0)
    rng, poses = T.scans(16, 90, 2)
    poses = poses.copy()
    poses[:, :3, 3] = [[0.1, 1.2, -0.5], [-0.4, 0.9, 0.3]]                      # inside the volume
    t0, w0 = T.fresh(shape)
    args = (origin, T.VOXEL, T.TRUNC, T.MAX_WEIGHT, rng * np.float32(0.25), poses)
    full = T.integrate(t0, w0, *args, max_range=3.0)
    same = T.integrate(t0, w0, *args, max_range=3.0, index_offset=(0, 0, 0))
    part = T.integrate(t0[8:, 2:, 4:], w0[8:, 2:, 4:], *args, max_range=3.0, index_offset=(4, 2, 8))
    assert (full["weight"] > 0).sum() > 200
    for k in ("tsdf", "weight"):
        assert np.array_equal(bits(same[k]), bits(full[k])) and np.array_equal(bits(part[k]), bits(full[k][8:, 2:, 4:]))

    d, w, org, vox, _ = T.sphere_volume()
    tri = T.triangles(d, w, org, vox)
    assert np.array_equal(bits(T.triangles(d, w, org, vox, index_offset=(0, 0, 0))), bits(tri))
    tail = T.triangles(d[8:], w[8:], org, vox, index_offset=(0, 0, 8))           # the cells with k >= 8 come last, in the same order
    assert 100 < len(tail) < len(tri) and np.array_equal(bits(tail), bits(tri[-len(tail):]))

    c = RC.volume_case("sphere")
    kw = dict(min_range=c["min_range"], max_range=c["max_range"], step=c["step"], min_weight=RC.MIN_WEIGHT)
    nz, ny, nx = c["tsdf"].shape
    big_t, big_w = T.fresh((nx + 16, ny + 16, nz + 16))
    big_t[8:8 + nz, 8:8 + ny, 8:8 + nx], big_w[8:8 + nz, 8:8 + ny, 8:8 + nx] = c["tsdf"], c["weight"]
    big_org = c["origin"] - 8 * c["voxel"]
    whole = RC.raycast(big_t, big_w, big_org, c["voxel"], c["poses"], 16, 90, **kw)
    block = RC.raycast(c["tsdf"], c["weight"], big_org, c["voxel"], c["poses"], 16, 90, index_offset=(8, 8, 8),
                       full_shape=(nx + 16, ny + 16, nz + 16), **kw)
    masked = RC.raycast(c["tsdf"], c["weight"], big_org, c["voxel"], c["poses"], 16, 90, index_offset=(8, 8, 8),
                        full_shape=(nx + 16, ny + 16, nz + 16), mask=RC.bricks(c["weight"], RC.MIN_WEIGHT), **kw)
    plain = RC.raycast(c["tsdf"], c["weight"], c["origin"], c["voxel"], c["poses"], 16, 90, **kw)
    zero = RC.raycast(c["tsdf"], c["weight"], c["origin"], c["voxel"], c["poses"], 16, 90, index_offset=(0, 0, 0), **kw)
    assert (whole["range"] > 0).sum() > 100
    for k in ("range", "vertex"):
        assert np.array_equal(bits(block[k]), bits(whole[k])) and np.array_equal(bits(masked[k]), bits(whole[k]))
        assert np.array_equal(bits(zero[k]), bits(plain[k]))


def test_semantic_dummy_and_tsdf_block_lie_where_the_cases_say():
    d = LX.SEMANTIC_DUMMY_POINTS
    assert (d - 1) * 20 < LX.B31 + 20 * 130000 and d * 20 >= LX.B31 and (d + 125000) * 20 * 4 <= 9e9
    c = LX.BY_NAME["tsdf_far_block"]
    (i0, j0, k0), e = LX.TSDF_BLOCK, LX.TSDF_BLOCK_EDGE
    assert k0 * c.per_item == LX.B30 and k0 + e == c.n and all(v % 8 == 0 for v in (i0, j0, k0, e))
    first = (k0 * 1024 + j0) * 1024 + i0
    assert first * 4 >= LX.B32 and all(t < 0 or t < LX.B30 for t in LX.truncations(first * 4))
