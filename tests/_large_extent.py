"""Shared by tests/test_gpu_large_extent.py (GPU) and tests/test_large_extent_host.py (CPU): the case table of the large-extent
tests as data, where the real items of a case go, what a truncated index would hit, and the guarded, sentinel-filled output
buffers with their on-device checks.

A case is one buffer of one entry point whose index passes 2^31 elements (or, where the header caps the element count below that,
whose byte offset passes 2^32).  The buffer holds `n` items of `per_item` elements of `elem_bytes` bytes each; almost all items are
empty, a few REAL ones sit at the places `real_items` names.  Nothing here imports torch at module level: the host test needs the
table and the arithmetic only."""
from collections import namedtuple

B30, B31, B32 = 1 << 30, 1 << 31, 1 << 32

GUARD_BYTES = 1 << 20
SENTINEL_I32 = 0x5A5A5A5A            # integer outputs: no kernel here writes this count, index or id
SENTINEL_F32_BITS = 0x7FC5A5A5       # float outputs: a quiet NaN with a payload; the kernels write finite values, -1 or +-inf

# entry: the exported call; buffer: the tensor whose index crosses; per_item: its elements per item (scan, volume, score, cell row);
# n: items; elem_bytes; crosses: the boundaries the case claims, in ELEMENTS of the buffer (B30 = byte offset 2^32 for 4-byte
# elements, B31 = index 2^31); cap: None, or the header's cap on the buffer's element count (then only B30 can be claimed).
Case = namedtuple("Case", "name entry buffer per_item n elem_bytes crosses cap")

HW = 64 * 900
CASES = [
    # ovn_project / ovn_normals at 64 x 900: q = scan * HW + pix, then q * C; the first four share one test (n = 12430: 31 GB)
    Case("project_vertex", "ovn_project", "vertex (n,H,W,4)", HW * 4, 12430, 4, (B30, B31), None),
    Case("project_stacked", "ovn_project", "stacked (n,H,W,4)", HW * 4, 12430, 4, (B30, B31), None),
    Case("normals_vertex_in", "ovn_normals", "vertex input (n,H,W,4)", HW * 4, 12430, 4, (B30, B31), None),
    Case("normals_out", "ovn_normals", "normal (n,H,W,3)", HW * 3, 12430, 4, (B30, B31), None),
    Case("project_normal", "ovn_project", "normal (n,H,W,3)", HW * 3, 12430, 4, (B30, B31), None),
    Case("project_range", "ovn_project", "range (n,H,W)", HW, 37290, 4, (B30, B31), None),
    Case("project_intensity", "ovn_project", "intensity (n,H,W)", HW, 37290, 4, (B30, B31), None),
    Case("project_keys", "ovn_project", "key image scratch (n,H,W) u64", HW, 37290, 8, (B30, B31), None),
    Case("gt_range", "ovn_gt_range_images", "range (n,H,W)", HW, 37290, 4, (B30, B31), None),
    Case("gt_counts_in", "ovn_gt_overlap_counts", "ref_ranges (n,H,W)", HW, 37290, 4, (B30, B31), None),
    # the leg: images (n,64,900,4) in, features (n,360,128) out; the 16 x 900 leg of INTEGRATION.md: (n,16,900,4) -> (n,371,128)
    Case("leg_input", "ovn_leg", "images (n,64,900,4)", HW * 4, 9325, 4, (B30, B31), None),
    Case("leg_output", "ovn_leg", "features (n,371,128)", 371 * 128, 45230, 4, (B30, B31), None),
    # one score per item; the header caps n at 2^31 - 1, so the index cannot cross: the byte offset does, and n sits 8 below the cap
    Case("top_k_scores", "ovn_top_k / ovn_best_match / ovn_top_k_segments", "overlap (n)", 1, B31 - 8, 4, (B30,), B31 - 1),
    # one grid row per item; the header caps nx * ny at 2^31 - 1
    Case("mcl_cells", "ovn_mcl_predict", "cell_frame (ny,nx)", 46340, 46340, 4, (B30,), B31 - 1),
    # the indexed / segmented head routes and the head backward calls gather 360 x 128 volumes out of a pool
    Case("heads_pool", "ovn_heads / ovn_delta_head / ovn_corr_head / ovn_heads_segments / ovn_delta_head_grad / ovn_heads_feature_grad",
         "feature pool (n,360,128)", 360 * 128, 46610, 4, (B30, B31), None),
    # ovn_render_scans at 64 x 900, q = (scan * H + y) * W + x
    Case("render_vertex", "ovn_render_scans", "vertex (n,H,W,4)", HW * 4, 9325, 4, (B30, B31), None),
    Case("render_stacked", "ovn_render_scans", "stacked (n,H,W,4)", HW * 4, 9325, 4, (B30, B31), None),
    # ovn_project_semantic at 20 classes: semantic (n,H,W,20), q * n_classes
    Case("semantic_out", "ovn_project_semantic", "semantic (n,H,W,20)", HW * 20, 1870, 4, (B30, B31), None),
    # the largest volume the header allows (nx ny nz <= 2^31 - 1): one x-y slab of samples per item
    Case("tsdf_volume", "ovn_tsdf_triangles (count) / ovn_tsdf_bricks", "tsdf, weight (nz,ny,nx)", 1290 * 1290, 1290, 4, (B30,), B31 - 1),
    # ovn_gt_pair_counts: counts (n_frames, n_refs) int32, the header caps the pairs at 2^31 - 1; one row of n_refs counts per item
    Case("gt_pair_counts", "ovn_gt_pair_counts", "counts (n_frames,n_refs)", 32769, 32769, 4, (B30,), B31 - 1),
    Case("semantic_stacked", "ovn_project_semantic", "stacked (n,H,W,25)", HW * 25, 1870, 4, (B30, B31), None),
    # ovn_tsdf_raycast at 64 x 900: the outputs of ovn_render_scans
    Case("raycast_vertex", "ovn_tsdf_raycast", "vertex (n,H,W,4)", HW * 4, 9325, 4, (B30, B31), None),
    Case("raycast_stacked", "ovn_tsdf_raycast", "stacked (n,H,W,4)", HW * 4, 9325, 4, (B30, B31), None),
    # the correlation head's (n, 360) output
    Case("corr_out", "ovn_corr_head / ovn_corr_head_spectral", "corr (n,360)", 360, 5965300, 4, (B30, B31), None),
    # a volume just past 2^30 samples (the header caps a volume at 2^31 - 1): one x-y slab of 1024 x 1024 samples per item
    Case("tsdf_far_block", "ovn_tsdf_integrate / ovn_tsdf_triangles / ovn_tsdf_bricks / ovn_tsdf_raycast", "tsdf, weight (nz,ny,nx)",
         1024 * 1024, 1072, 4, (B30,), B31 - 1),
]
BY_NAME = {c.name: c for c in CASES}


def straddler(per_item, boundary):
    """The item that holds element `boundary` (it STRADDLES the boundary unless it starts exactly there)."""
    return boundary // per_item


def real_items(case):
    """Sorted item indices that hold real data: 0, the item that straddles each claimed boundary and the one after it, the last."""
    want = {0, case.n - 1}
    for b in case.crosses:
        s = straddler(case.per_item, b)
        want.update((s, s + 1))
    return sorted(i for i in want if 0 <= i < case.n)


def extent(case, item):
    return item * case.per_item, (item + 1) * case.per_item


def truncations(offset):
    """What a 32-bit index would make of `offset`: reduced mod 2^32, and that reinterpreted as a signed 32-bit integer.  Only the
    values that differ from the offset itself (a correct index is no truncation)."""
    lo = offset % B32
    signed = lo - B32 if lo >= B31 else lo
    return sorted({v for v in (lo, signed) if v != offset})


def truncated_targets(case, item):
    """For a real item: (kind, wrong offset, what it hits) for a truncated ELEMENT offset of its first and last element and for a
    truncated BYTE offset of the same two (reported in elements).  'hits' is 'outside' (before the buffer: the front guard or a
    fault), 'empty' (an item that must keep its empty value), 'real' (another real item, whose bits would change) or 'own'."""
    reals = set(real_items(case))
    out = []
    lo, hi = extent(case, item)
    for kind, scale in (("element", 1), ("byte", case.elem_bytes)):
        for off in (lo, hi - 1):
            for t in truncations(off * scale):
                e = t // scale if t >= 0 else -((-t) // scale) - 1
                if e < 0 or e >= case.n * case.per_item:
                    hit = "outside"
                elif lo <= e < hi:
                    hit = "own"
                else:
                    hit = "real" if e // case.per_item in reals else "empty"
                out.append((kind, e, hit))
    return out


# ovn_project on two scans, the first a dummy of this many points at the origin (the range filter drops depth 0): the second scan's
# points start at element PROJECT_DUMMY_POINTS * 4 of `points`, past 2^31, and its kept-point numbering at byte 2^31 of the scratch
PROJECT_DUMMY_POINTS = 537000000

# ovn_project_semantic on two scans, the first a dummy of this many points at the origin: the real scan's probability rows start at
# element SEMANTIC_DUMMY_POINTS * 20, past 2^31
SEMANTIC_DUMMY_POINTS = 107400000

# the block of the tsdf_far_block volume that the scans touch: (i0, j0, k0) and its edge; k0 * 1024 * 1024 == 2^30
TSDF_BLOCK = (488, 488, 1024)
TSDF_BLOCK_EDGE = 48

# ovn_leg_forward_train / ovn_leg_backward keep the activations LAYER-MAJOR: block li = (n, act[li]) at n * (act[0] + .. + act[li-1]).
# The real scans are the first and the last LEG_TRAIN_BLOCK scans (whole scan blocks of the backward pass), everything between is empty.
LEG_TRAIN_N = 2260
LEG_TRAIN_BLOCK = 4


def leg_activation_sizes(in_h, in_w, in_c, cfg):
    """Elements per scan of every leg layer's output (what ovn_leg_activation_sizes returns), from the layer table."""
    from overlapnet_amd import weights as WT
    h, w, out = in_h, in_w, []
    for l in WT.leg_layers(in_c, cfg):
        h, w = (h - l.kh) // l.sh + 1, (w - l.kw) // l.sw + 1
        out.append(h * w * l.cout)
    return out


# ---- device side (torch imported on use) -----------------------------------------------------------------------------------------

CHUNK = 1 << 27          # elements per pass of an on-device check: no temporary of a check is larger than 128 Mi elements


class Guarded(object):
    """An output tensor of 4-byte elements that is a view INSIDE a larger allocation: GUARD_BYTES in front and behind, everything
    pre-filled with the sentinel of its type."""

    def __init__(self, shape, dtype, device):
        import torch
        assert dtype in (torch.float32, torch.int32)
        self.numel = 1
        for s in shape:
            self.numel *= int(s)
        g = GUARD_BYTES // 4
        bits = SENTINEL_F32_BITS if dtype == torch.float32 else SENTINEL_I32
        self.sentinel = bits
        self.raw = torch.empty(self.numel + 2 * g, dtype=torch.int32, device=device)
        for a in range(0, self.raw.numel(), CHUNK):
            self.raw[a:a + CHUNK].fill_(bits)
        self.bits = self.raw[g:g + self.numel]                      # the output as int32 words, flat
        self.t = self.bits.view(dtype).view(*shape)                 # the tensor handed to the library
        self.front, self.back = self.raw[:g], self.raw[g + self.numel:]
        self.bytes = self.raw.numel() * 4

    def guards_intact(self):
        return bool((self.front == self.sentinel).all().item()) and bool((self.back == self.sentinel).all().item())

    def count_not(self, value_bits, lo=0, hi=None):
        """Number of 32-bit words in [lo, hi) of the flat output that differ from value_bits."""
        hi = self.numel if hi is None else hi
        bad = 0
        for a in range(lo, hi, CHUNK):
            bad += int((self.bits[a:min(a + CHUNK, hi)] != value_bits).sum().item())
        return bad

    def count_sentinel(self):
        return self.numel - self.count_not(self.sentinel)


def f32_bits(x):
    import struct
    return struct.unpack("<i", struct.pack("<f", x))[0]


def check_items(g, per_item, n, reals, small_bits, empty_bits):
    """Checks (a), (b), (c) on a Guarded output of n items of per_item words: both guards intact; real item reals[j] == row j of
    small_bits (int32 words, (len(reals), per_item)) bit for bit; every other item == empty_bits (a scalar word or a row of per_item
    words).  Returns a dict of counts; the caller asserts that all are zero / True."""
    res = {"guards": g.guards_intact(), "sentinel_left": g.count_sentinel()}
    res.update(check_rows(g.bits.view(n, per_item), reals, small_bits, empty_bits))
    return res


def check_rows(view, reals, small_bits, empty_bits):
    """(b) and (c) on an (n, per_item) int32 view: {'real_diff', 'empty_diff'} word counts."""
    import torch
    n, per_item = view.shape
    res = {"real_diff": 0, "empty_diff": 0}
    for j, i in enumerate(reals):
        res["real_diff"] += int((view[i] != small_bits[j].reshape(-1)).sum().item())
    edges = [-1] + list(reals) + [n]
    rows = max(1, CHUNK // per_item)
    for a, b in zip(edges[:-1], edges[1:]):
        for r0 in range(a + 1, b, rows):
            blk = view[r0:min(r0 + rows, b)]
            if torch.is_tensor(empty_bits):
                res["empty_diff"] += int((blk != empty_bits.reshape(1, -1)).sum().item())
            else:
                res["empty_diff"] += int((blk != empty_bits).sum().item())
    return res


def need_or_skip(need_bytes):
    """Skip (with the byte counts) only when the device has less free memory than the case needs plus 10 %."""
    import pytest
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < need_bytes * 1.1:
        pytest.skip("needs %d bytes (+ 10 %%), the device has %d free" % (need_bytes, free))


def release():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()
