"""GPU (MI355X): entry points run where an index of theirs passes 2^31 elements or a byte offset passes 2^32.

Every other test keeps every `scan * H * W + pix`, `s0 * in_elems`, `iy * nx + ix` below 2^20; here the buffers are multi-gigabyte
and almost entirely EMPTY (scans without points, all -1 leg images, zero scores, cells without a frame), with a few REAL items
(the fixtures the modules' own tests use) at item 0, at the item that straddles 2^30 elements (byte offset 2^32) and the one after
it, at the item that straddles 2^31 elements and the one after it, and at the last item (tests/_large_extent.py: `real_items`;
tests/test_large_extent_host.py checks that arithmetic and what a truncated index would hit).  Every large output is a view inside
a larger allocation with 1 MiB guard bands, all pre-filled with a sentinel no kernel writes.  Checked on the device:
  (a) both guards intact;  (b) the real items' outputs == one small call on those items alone, bit for bit (the header's promise:
  a scan's result does not depend on the batch -- which the modules' own tests tie to the fp64 references);  (c) every other item
  holds exactly the empty value: no sentinel left, no stray write in bounds;  (d) where the host reference takes well under a second,
  the LAST item against it at the module's existing tolerance.
Each test prints its time and peak memory (torch allocations + the context's scratch).

Audit (read before any run).  "limit" is what include/ovn_hip.h states; every product below is formed in 64 bits unless said.

entry point            | buffer                    | expression (file:line)                                        | limit                 | case / why it cannot cross
-----------------------+---------------------------+---------------------------------------------------------------+-----------------------+---------------------------
ovn_project            | key image (scratch)       | (long long)scan*gm.H*gm.W + pix      projection.hip:88        | n <= 65535, HW < 2^31 | project_keys (n = 37290)
ovn_project            | keys / range / intensity  | q = (long long)scan*HW + pix         projection.hip:181-182   | same                  | project_range, project_intensity
ovn_project            | vertex, stacked (C = 4)   | q * 4, q * C                         projection.hip:211,220   | same                  | project_vertex, project_stacked (n = 12430)
ovn_project            | normal                    | q * 3                                projection.hip:215-217   | same                  | project_normal (n = 12430)
ovn_project            | idx, local_idx, block_cnt | scan*max_points + p, scan*blocks_per_scan + b  :99,103,194    | < 2^32 points a scan  | project points (537 M dummy points)
ovn_project            | points                    | (beg + p) * 4, offsets[scan] * 4     projection.hip:64,183    | int64 offsets         | project points (the same case)
ovn_project            | H * W, pix = py * W + px  | int                                  projection.hip:158,180   | was UNSTATED          | refusal: H*W <= 2^31 - 1 (host test)
ovn_project            | grid (blocks, n_scans)    | dim3 y                               projection.hip:347       | was UNSTATED          | refusal: n_scans <= 65535 (host test)
ovn_project_semantic   | same kernels' twins       | projection.hip:410,418-419,427,484-486,512,540,553            | n <= 65535 (stated)   | semantic_out, semantic_stacked (n = 1870); semantic rows (107.4 M dummy points: probs rows past 2^31); H*W refusal
ovn_projection_angles  | pixel = py * W + px       | proj_pixel.h (point_to_pixel), int                            | was UNSTATED          | refusal: H*W <= 2^31 - 1 (host test)
ovn_normals            | range / vertex / normal   | q, q * 4, q * 3 (q long long)        projection.hip:244-280   | was UNSTATED (H * W)  | normals_vertex_in, normals_out (n = 12430); refusal
ovn_icp_register       | range / vertex / normal   | (size_t)si*HW [*4, *3]               icp_register.hip:212-217 | HW <= 2^31 - 1        | pairs (n-1, n-2) vs (1, 0) on project_vertex's images
ovn_gt_range_images    | range                     | (long long)s*H*W + pix               overlap_gt.hip:83        | n <= 65535            | gt_range (n = 37290)
ovn_gt_range_images    | pix = (int)py*W + (int)px | int                                  overlap_gt.hip:64        | was UNSTATED          | refusal: H*W <= 2^31 - 1 (host test)
ovn_gt_overlap_counts  | ref_ranges                | (long long)s * npix                  overlap_gt.hip:158       | was UNSTATED (H * W)  | gt_counts_in (n = 37290); refusal
ovn_gt_overlap_counts  | pixel loops               | int i = threadIdx.x; i += 256        overlap_gt.hip:160,165   | H*W <= 2^31 - 1       | TRUNCATED, fixed (see below); NOT RUN at the cap: one 256-thread workgroup over 2 x 8.6 GB, more than 10 s at the rate ovn_best_match's 1024 threads show
ovn_gt_overlap_counts  | grid n + 1                | int                                  overlap_gt.hip:196       | was UNSTATED          | refusal: n_scans <= 2^31 - 2 (host test)
ovn_gt_pair_counts     | counts                    | (long long)fi*n_refs + ri            overlap_gt.hip:110       | pairs <= 2^31 - 1     | gt_pair_counts (32 769^2 pairs): bytes pass 2^32
ovn_gt_pair_counts     | cur_ranges, points, poses | cur_ranges + (long long)f*npix, points + 4*i (long long i), 16*(long long)r   overlap_gt.hip:117-122 | H*W <= 262144 | gt_pair_counts (cur_ranges of 32 769 scans: 1.9e9 floats, bytes pass 2^32); int npix, words <= 8192: cannot cross
ovn_icp_register       | pose, stats, system       | 16 * pair, 8 * pair, 28 * pair (size_t pair)   icp_register.hip:201-207 | n_pairs < 2^31   | cannot cross in elements below 2^27 pairs; the (n-1, n-2) pairs run with guarded outputs
ovn_icp_register       | pixel groups              | int g < groups = (HW + 3) >> 2; p0 = 4*(int64)g   icp_register.hip:211,239-240 | HW <= 2^31 - 1 | cannot cross: groups <= 2^29
ovn_leg                | images                    | (size_t)s0 * in_elems                ovn_api.hip:361          | none (int64 n)        | leg_input (n = 9325), f16x3 and f32
ovn_leg                | features                  | (size_t)s0 * feat_elems              ovn_api.hip:378,395      | none                  | leg_output (16 x 900 -> 371, n = 45230)
ovn_leg                | slice scratch, actmax     | slice * max_act, (li + 2)*slice*STRIDE   ovn_api.hip:351,384  | slice <= 1024 scans   | cannot cross: 1024 * 197 k floats = 2.0e8 elements
ovn_top_k              | overlap                   | int i = tail + threadIdx.x; i += 1024    top_k.hip:67         | n <= 2^31 - 1         | top_k_scores: TRUNCATED, fixed (see below)
ovn_best_match         | overlap                   | int k = threadIdx.x; k += 1024       best_match.hip:36        | n <= 2^31 - 1         | top_k_scores: TRUNCATED, fixed (see below)
ovn_top_k_segments     | overlap + offs[b]         | int64 base; n = (int)(offs[b+1] - base)  top_k.hip:78-84      | offs[B] <= 2^31 - 1   | top_k_scores (a segment of 2^31 - 16 scores); offsets past 2^31 are refused (ovn_api.hip:1132)
ovn_mcl_predict        | cell_frame                | (size_t)iy * g.nx + ix               mcl.hip:93               | nx * ny <= 2^31 - 1   | mcl_cells: the byte offset passes 2^32; the index cannot pass 2^31
ovn_heads, ovn_delta_head, ovn_corr_head, ovn_heads_segments, ovn_delta_head_grad, ovn_heads_feature_grad
                       | feature pools             | feats + (size_t)lidx[p] * vol (int32 index, 64-bit product in   | int32 indices         | heads_pool (46 610 volumes, the last
                       |                           | every kernel that gathers a volume)                           |                       | four past 2^31), f16x3 and f32
ovn_render_scans       | range, tri_id, vertex     | q = (scan*H + y)*(long long)W + x; q * 4   render_mesh.hip:98,125-129 | HW <= 2^31 - 1   | render_vertex (n = 9325), both routes
ovn_render_scans       | normal, stacked           | s0*HW*3, s0*HW*C, then proj_normal_kernel  render_mesh.hip:298-300    | same             | render_stacked
ovn_render_scans       | grid ns * tiles_per_scan  | at most 2^30 tiles a launch                render_mesh.hip:266,290    | same             | cannot cross: one launch per 2^30 tiles
ovn_leg_forward_train  | acts (layer-major)        | dst += (size_t)n * g.act[li]         ovn_api.hip:477          | n < 2^31              | leg train (n = 2260: 2.15e9 activations)
ovn_leg_forward_train  | one layer, all n scans    | m, abase in long long                conv_f32.hip:74-89       | n < 2^31              | NOT RUN: one layer past 2^31 needs n = 9321 and 60 GB of activations
ovn_leg_backward       | acts, dfeat, images       | (size_t)n*act_off[li] + (size_t)s0*g.act[li]   ovn_api.hip:515,520 | n < 2^31           | leg train (the same buffer)
ovn_leg_backward       | slice scratch, partials   | nmax * g.act_max, part_bytes         ovn_api.hip:497-499      | slice <= 65532 scans  | cannot cross at the default slice of 32 scans
ovn_tsdf_triangles     | tsdf, weight              | s = ((long long)(k+dz)*ny + j+dy)*nx + i+dx   tsdf.hip:216,253  | nx ny nz <= 2^31 - 1  | tsdf_volume (1290^3, count mode): bytes pass 2^32, the index cannot pass 2^31
ovn_tsdf_bricks        | weight, mask              | the same sample index; one byte per 8^3 brick                   | same                  | tsdf_volume
ovn_tsdf_integrate     | tsdf, weight, range       | idx = ((long long)k*ny + j)*nx + i; (long long)s*HW + row*W + col   tsdf.hip:124,145   | nx ny nz <= 2^31 - 1  | tsdf_far_block (1024 x 1024 x 1072; the block at slab 1024 = sample 2^30)
ovn_tsdf_integrate     | waves, grid               | wave = (long long)blockIdx.x*4 + ..; blocks < 2^31   tsdf.hip:109,346     | same                  | cannot cross (the comment at tsdf.hip:346)
ovn_tsdf_triangles     | triangles (write mode)    | g = wg[blockIdx.x] + before (long long)   tsdf.hip:237                 | capacity int64        | tsdf_far_block (write mode into a guarded buffer)
ovn_tsdf_raycast       | tsdf, weight, bricks      | base = (long long)kk*sz + (long long)j*sy + i; brick index in long long   tsdf_raycast.hip:71,85-87 | same    | tsdf_far_block, without and with the mask
ovn_tsdf_raycast       | range, vertex, normal, stacked | q = (scan*H + y)*(long long)W + x; s0*HW*C   tsdf_raycast.hip:49,224-230 | HW <= 2^31 - 1  | raycast_vertex, raycast_stacked (n = 9325), both routes
ovn_tsdf_bricks        | weight, mask (far block)  | ((long long)k*ny + j)*nx + i   tsdf_raycast.hip:146,152                  | same                  | tsdf_far_block
ovn_corr_head, ovn_corr_head_spectral | corr (n, 360), yaw | corr[(long long)pair*W + tid], corr_out + (long long)pair*FW   corr_head.hip:148, corr_spectral.hip:171 | n int64 (int pair) | corr_out (5 965 300 pairs, every row compared)

Truncation found and fixed: the score loops of ovn_top_k (the tail loop of for_each_score, top_k.hip:67) and ovn_best_match
(best_match.hip:36) counted in `int`.  With n within 1024 of 2^31 - 1, which the header allows, `tail + threadIdx.x` resp. the
last `k += 1024` passes 2^31 - 1, wraps negative, is still "< n" and reads up to 8 GB in front of the scores.  The counters are
uint32_t now.  test_top_k_best_match_and_segments runs n = 2^31 - 8 (tail = n, so threads 8..1023 wrapped at once).

Truncation found on review and fixed: gt_count_kernel's two pixel loops (overlap_gt.hip:160,165) counted in `int`; with H*W within
256 of 2^31 - 1, which ovn_gt_overlap_counts accepts, the counter wrapped negative and read in front of the images.  uint32_t now.

Left out: one layer of ovn_leg_forward_train past 2^31 (audited; 60 GB of activations, over the 40 GB of a test), and
ovn_gt_overlap_counts at H*W = 2^31 - 1 (one 256-thread workgroup walks 2 x 8.6 GB: more than ten seconds).

Measured on an MI355X, none skipped, 27 s for the module's 22 cases: the figures per case are in DESIGN.md section 35."""
import time

import numpy as np
import pytest
import torch

import _large_extent as LX
import _mcl_ref as MR
from oracle import overlapnet_oracle as O
from overlapnet_amd import _lib
from overlapnet_amd.engine import _ptr
from tools import synthetic as S

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

H, W = 64, 900
HW = H * W
GEO = (3.0, -25.0, 50.0)
M1 = LX.f32_bits(-1.0)
GB = 1e9


class _Meter(object):
    """Time and peak memory of one case, printed when it ends."""

    def __init__(self, name, eng):
        self.name, self.eng = name, eng

    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        dt = time.perf_counter() - self.t0
        peak = torch.cuda.max_memory_allocated()
        ws = self.eng.workspace_bytes() if self.eng is not None and getattr(self.eng, "_h", None) else 0
        print("[large extent] %s: %.2f s, peak %.2f GB torch + %.2f GB library scratch = %.2f GB"
              % (self.name, dt, peak / GB, ws / GB, (peak + ws) / GB))
        return False


@pytest.fixture()
def eng():
    """A fresh context per test: its scratch (the 17 GB key image of the largest projection) goes with it."""
    from overlapnet_amd.engine import OvnEngine
    e = OvnEngine(H, W, 4, device=0)
    yield e
    e.close()
    LX.release()


def _clouds(fixture_npz, reals, pinned=None):
    """One cloud per real item: the two fixture scans alternately, each turned about z by its own number of columns so that no two
    items hold the same data.  pinned: {item: (fixture scan, columns)} overrides."""
    out = []
    for j, i in enumerate(reals):
        s, c = (pinned or {}).get(i, (j % 2, 37 * (j + 1)))
        out.append(S.z_rotated(fixture_npz["points_%d" % s], c))
    return out


def _batch(clouds, reals, n, dev):
    """points (total, 4) and offsets (n + 1): scan reals[j] = clouds[j], every other scan has no points."""
    counts = np.zeros(n, np.int64)
    counts[np.asarray(reals)] = [len(c) for c in clouds]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds).astype(np.float32))).to(dev)
    return pts, torch.from_numpy(offs).to(dev), int(counts.max())


def _small(eng, clouds, want, stacked_flags=None):
    pts, offs, mx = _batch(clouds, list(range(len(clouds))), len(clouds), eng.device)
    return eng.project(pts, offs, mx, H, W, *GEO, want=want, stacked_flags=stacked_flags)


def _project(eng, pts, offs, n, mx, rng=None, vtx=None, itn=None, idx=None, nrm=None, stk=None, flags=(0, 0, 0)):
    _lib.check(eng.lib.ovn_project(eng._h, _ptr(pts), _ptr(offs), n, mx, H, W, *GEO, _ptr(rng), _ptr(vtx), _ptr(itn), _ptr(idx),
                                   _ptr(nrm), _ptr(stk), flags[0], flags[1], flags[2], eng._stream()), "ovn_project")


def _bits(t):
    return t.contiguous().view(torch.int32).reshape(t.shape[0], -1)


def _guarded64(shape, dtype, dev):
    """A guarded float64 / int64 output: (Guarded of the int32 words, the tensor to hand to the library)."""
    g = LX.Guarded((2 * int(np.prod(shape)),), torch.int32, dev)
    return g, g.bits.view(dtype).view(*shape)


def _assert_clean(tag, res):
    print("[large extent]   %s: %s" % (tag, res))
    assert res["guards"], tag + ": a guard band was written"
    assert res["real_diff"] == 0, tag + ": a real item differs from the small call"
    assert res["empty_diff"] == 0 and res["sentinel_left"] == 0, tag + ": an empty item does not hold the empty value"


def _reals(name, extra=()):
    c = LX.BY_NAME[name]
    return c, sorted(set(LX.real_items(c)) | set(extra))


# ---- ovn_project, ovn_normals, ovn_icp_register ------------------------------------------------------------------------------------

def test_project_vertex_stacked_then_normals_and_icp(eng, fixture_npz):
    """q * 4 (vertex and the stacked C = 4 leg input) past 2^31; ovn_normals reads that vertex image and writes q * 3 past 2^31 too
    (real items at the boundaries of both layouts);
    ovn_icp_register on these images: the pairs (n - 1, n - 2) and (1, 0) hold the same two scans and must give the same bits."""
    c, reals = _reals("project_vertex", extra=[1, LX.BY_NAME["project_vertex"].n - 2] + LX.real_items(LX.BY_NAME["normals_out"]))
    n = c.n
    assert n == LX.BY_NAME["normals_out"].n == LX.BY_NAME["project_stacked"].n
    LX.need_or_skip(int(34e9))
    pinned = {0: (0, 0), 1: (1, 0), n - 2: (0, 0), n - 1: (1, 0)}          # the pair (1, 0) of tests/test_gpu_icp.py, twice
    clouds = _clouds(fixture_npz, reals, pinned)
    dev = eng.device
    with _Meter("project vertex + stacked, normals, icp (n = %d)" % n, eng):
        pts, offs, mx = _batch(clouds, reals, n, dev)
        g_vtx, g_stk = LX.Guarded((n, H, W, 4), torch.float32, dev), LX.Guarded((n, H, W, 4), torch.float32, dev)
        g_rng = LX.Guarded((n, H, W), torch.float32, dev)
        _project(eng, pts, offs, n, mx, rng=g_rng.t, vtx=g_vtx.t, stk=g_stk.t, flags=(1, 1, 0))
        small = _small(eng, clouds, ("range", "vertex", "normal"), (1, 1, 0))
        _assert_clean("vertex", LX.check_items(g_vtx, HW * 4, n, reals, _bits(small["vertex"]), M1))
        _assert_clean("stacked", LX.check_items(g_stk, HW * 4, n, reals, _bits(small["stacked"]), M1))
        _assert_clean("range", LX.check_items(g_rng, HW, n, reals, _bits(small["range"]), M1))
        # (d) the last item against the oracle, bit for bit as in tests/test_gpu_parity.py
        o_rng, o_vtx, _, _ = O.range_projection(clouds[-1])
        o_nrm = O.gen_normal_map(o_rng, o_vtx)
        assert np.array_equal(g_rng.t[n - 1].cpu().numpy(), o_rng) and np.array_equal(g_vtx.t[n - 1].cpu().numpy(), o_vtx)
        assert np.array_equal(g_stk.t[n - 1].cpu().numpy(), np.concatenate([o_rng[..., None], o_nrm], axis=-1))
        del g_stk
        LX.release()

        g_nrm = LX.Guarded((n, H, W, 3), torch.float32, dev)
        _lib.check(eng.lib.ovn_normals(eng._h, _ptr(g_rng.t), _ptr(g_vtx.t), n, H, W, _ptr(g_nrm.t), eng._stream()), "ovn_normals")
        small_n = eng.normals(small["range"], small["vertex"])
        assert torch.equal(_bits(small_n), _bits(small["normal"]))
        _assert_clean("ovn_normals", LX.check_items(g_nrm, HW * 3, n, reals, _bits(small_n), M1))
        assert np.array_equal(g_nrm.t[n - 1].cpu().numpy(), o_nrm)
        assert g_vtx.guards_intact() and g_rng.guards_intact()

        pairs = torch.tensor([[n - 1, n - 2], [1, 0]], dtype=torch.int32, device=dev)
        T0 = torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1).contiguous()
        (gp, pose), (gs_, stats), (gy, system) = (_guarded64(sh, torch.float64, dev) for sh in ((2, 4, 4), (2, 8), (2, 28)))
        src, tgt = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()         # held: a pointer does not keep a temporary alive
        _lib.check(eng.lib.ovn_icp_register(eng._h, _ptr(g_vtx.t), _ptr(g_nrm.t), _ptr(g_rng.t), n, H, W, *GEO,
                                            _ptr(src), _ptr(tgt), 2, _ptr(T0), 5, 2.0, 0.8, 0.2,
                                            64, _ptr(pose), _ptr(stats), _ptr(system), eng._stream()), "ovn_icp_register")
        assert gp.guards_intact() and gs_.guards_intact() and gy.guards_intact() and gp.count_sentinel() == 0
        sp, ss, sy = eng.icp_register(small["vertex"], small["normal"], small["range"],
                                      torch.tensor([reals.index(n - 1), 1], dtype=torch.int32, device=dev),
                                      torch.tensor([reals.index(n - 2), 0], dtype=torch.int32, device=dev), T0, iterations=5,
                                      want_system=True)
        for big, sm in ((pose, sp), (stats, ss), (system, sy)):
            b = big.view(torch.int64).reshape(2, -1)
            assert torch.equal(b[0], b[1]) and torch.equal(b, sm.view(torch.int64).reshape(2, -1))
        assert float(stats[0, 0]) == 0.0 and float(stats[0, 2]) > 1000          # a real registration, not two refusals
        del g_vtx, g_rng, g_nrm, pts, offs, small, small_n
    LX.release()


def test_project_normal_past_2_31(eng, fixture_npz):
    c, reals = _reals("project_normal")
    n = c.n
    LX.need_or_skip(int(17e9))
    clouds = _clouds(fixture_npz, reals)
    dev = eng.device
    with _Meter("project normal (n = %d)" % n, eng):
        pts, offs, mx = _batch(clouds, reals, n, dev)
        g = LX.Guarded((n, H, W, 3), torch.float32, dev)
        _project(eng, pts, offs, n, mx, nrm=g.t)
        small = _small(eng, clouds, ("range", "vertex", "normal"))
        _assert_clean("normal", LX.check_items(g, HW * 3, n, reals, _bits(small["normal"]), M1))
        o_rng, o_vtx, _, _ = O.range_projection(clouds[-1])
        assert np.array_equal(g.t[n - 1].cpu().numpy(), O.gen_normal_map(o_rng, o_vtx))
        del g, pts, offs, small
    LX.release()


def test_project_range_intensity_past_2_31(eng, fixture_npz):
    """q itself past 2^31: the range and intensity images, and a key image of 17 GB in the context's scratch."""
    c, reals = _reals("project_range")
    n = c.n
    LX.need_or_skip(int(38e9))
    clouds = _clouds(fixture_npz, reals)
    dev = eng.device
    with _Meter("project range + intensity (n = %d)" % n, eng):
        pts, offs, mx = _batch(clouds, reals, n, dev)
        g_rng, g_itn = LX.Guarded((n, H, W), torch.float32, dev), LX.Guarded((n, H, W), torch.float32, dev)
        _project(eng, pts, offs, n, mx, rng=g_rng.t, itn=g_itn.t)
        small = _small(eng, clouds, ("range", "intensity"))
        _assert_clean("range", LX.check_items(g_rng, HW, n, reals, _bits(small["range"]), M1))
        _assert_clean("intensity", LX.check_items(g_itn, HW, n, reals, _bits(small["intensity"]), M1))
        o_rng, _, o_itn, _ = O.range_projection(clouds[-1])
        assert np.array_equal(g_rng.t[n - 1].cpu().numpy(), o_rng) and np.array_equal(g_itn.t[n - 1].cpu().numpy(), o_itn)
        del g_rng, g_itn, pts, offs, small
    LX.release()


# ---- ovn_gt_range_images, ovn_gt_overlap_counts -------------------------------------------------------------------------------------

def test_gt_range_images_and_overlap_counts_past_2_31(eng, fixture_npz):
    import _gt_pairs_ref as GR
    c, reals = _reals("gt_range")
    n = c.n
    LX.need_or_skip(int(10e9))
    clouds = _clouds(fixture_npz, reals)
    dev = eng.device
    with _Meter("gt range images + overlap counts (n = %d)" % n, eng):
        pts, offs, mx = _batch(clouds, reals, n, dev)
        g = LX.Guarded((n, H, W), torch.float32, dev)
        _lib.check(eng.lib.ovn_gt_range_images(eng._h, _ptr(pts), _ptr(offs), n, mx, None, None, H, W, *GEO, _ptr(g.t), eng._stream()),
                   "ovn_gt_range_images")
        sp, so, smx = _batch(clouds, list(range(len(clouds))), len(clouds), dev)
        small = eng.gt_range_images(sp, so, smx)
        _assert_clean("gt range", LX.check_items(g, HW, n, reals, _bits(small), M1))
        ref = O.range_image_f64(GR.homog(clouds[-1][:, :3]))
        diff = int(np.count_nonzero(g.t[n - 1].cpu().numpy() != ref))
        print("[large extent]   last item vs the float64 oracle: %d pixels differ (allowed 4, tests/test_gpu_parity.py)" % diff)
        assert diff <= 4

        cur = small[0].contiguous()
        gc_ = LX.Guarded((n + 1,), torch.int32, dev)
        _lib.check(eng.lib.ovn_gt_overlap_counts(eng._h, _ptr(g.t), _ptr(cur), n, H, W, _ptr(gc_.t), eng._stream()),
                   "ovn_gt_overlap_counts")
        sc = eng.gt_overlap_counts(small, cur)                              # (k + 1): the real items, then #{cur > 0}
        _assert_clean("gt counts", LX.check_items(gc_, 1, n + 1, reals + [n], sc.reshape(-1, 1), 0))
        last, cur_h = g.t[n - 1].cpu().numpy(), cur.cpu().numpy()
        assert int(gc_.t[n - 1]) == int(np.count_nonzero((last > 0) & (np.abs(last - cur_h) < 1)))
        assert int(gc_.t[n]) == int(np.count_nonzero(cur_h > 0)) and int(gc_.t[0]) == int(gc_.t[n])
        assert g.guards_intact()
        del g, gc_, pts, offs, small
    LX.release()


# ---- ovn_leg ------------------------------------------------------------------------------------------------------------------------

def _leg_case(name, h, w, cfg, feat_w, precisions, fixture_npz, need):
    from overlapnet_amd.engine import OvnEngine
    c, reals = _reals(name)
    n = c.n
    LX.need_or_skip(need)
    e = OvnEngine(h, w, 4, device=0)
    try:
        e.load_weights(S.make_test_weights(4, model_cfg=cfg, feat_w=feat_w), cfg)
        assert e.feat_w == feat_w
        dev = e.device
        step = H // h
        real = np.stack([np.roll(S.stack(fixture_npz["range_%d" % (j % 2)], fixture_npz["normal_%d" % (j % 2)],
                                         fixture_npz["intensity_%d" % (j % 2)], S.flags_of(4))[::step], 37 * j, axis=1)
                         for j in range(len(reals))])
        with _Meter("%s (n = %d, %d x %d, %s)" % (name, n, h, w, "/".join(precisions)), e):
            imgs = torch.empty((n, h, w, 4), dtype=torch.float32, device=dev)
            rows = max(1, LX.CHUNK // (h * w * 4))
            for a in range(0, n, rows):
                imgs[a:a + rows].fill_(-1.0)                                # an empty scan: every pixel -1
            small_in = torch.from_numpy(np.concatenate([real, np.full((1, h, w, 4), -1, np.float32)])).to(dev)
            imgs[torch.tensor(reals, device=dev)] = small_in[:-1]
            for prec in precisions:
                e.set_leg_precision(prec)
                g = LX.Guarded((n, feat_w, 128), torch.float32, dev)
                e.leg(imgs, out=g.t)
                small = _bits(e.leg(small_in))
                assert bool(torch.isfinite(small.view(torch.float32)).all())
                _assert_clean("features " + prec, LX.check_items(g, feat_w * 128, n, reals, small[:-1], small[-1]))
                del g
                LX.release()
            del imgs, small_in
    finally:
        e.close()
        LX.release()


def test_leg_input_offset_past_2_31(fixture_npz):
    """s0 * in_elems: 9325 images of 64 x 900 x 4, in both leg precisions (f16x3 also indexes actmax per scan of a slice).  The empty
    value of a feature volume is the leg's output on an all -1 image, taken from the small call."""
    _leg_case("leg_input", 64, 900, S.REFERENCE_MODEL_CFG, 360, ("f16x3", "f32"), fixture_npz, int(14e9))


def test_leg_output_offset_past_2_31(fixture_npz):
    """s0 * feat_elems: the documented 16 x 900 -> 371-column leg, 45 230 scans."""
    import _leg_geometry_ref as G
    strides, a3, (h, w), fw = G.DOCUMENTED
    _leg_case("leg_output", h, w, G.cfg_of(strides, a3, (h, w), fw), fw, ("f16x3",), fixture_npz, int(22e9))


# ---- ovn_top_k, ovn_best_match, ovn_top_k_segments ----------------------------------------------------------------------------------

def test_top_k_best_match_and_segments(eng):
    """n = 2^31 - 8 zero scores with planted winners at the first position, around 2^30 and at the last positions; the maximal
    index_offset (7).  k = 8 takes the six winners and then the two first zeros: the tie rule walks the position digits of all
    2^31 - 8 scores.  The records are known in closed form."""
    c = LX.BY_NAME["top_k_scores"]
    n, k, off, thr = c.n, 8, 7, 0.3
    LX.need_or_skip(int(9e9))
    dev = eng.device
    plant = [(0, 0.25), (LX.B30 - 1, 0.9), (LX.B30, 0.85), (LX.B30 + 1, 0.95), (n - 2, 0.5), (n - 1, 0.75)]
    with _Meter("top_k / best_match / top_k_segments (n = 2^31 - 8)", eng):
        scores = torch.zeros(n, dtype=torch.float32, device=dev)
        for p, v in plant:
            scores[p] = v
        order = sorted(plant, key=lambda pv: -pv[1])

        def records(items, shift, base):
            return np.array([[p - base + shift, LX.f32_bits(v), 0, 1 if np.float32(v) > np.float32(thr) else 0] for p, v in items],
                            np.int32)

        want = np.concatenate([records(order, off, 0), records([(1, 0.0), (2, 0.0)], off, 0)])
        g = LX.Guarded((k, 4), torch.int32, dev)
        eng.top_k(scores, k=k, threshold=thr, index_offset=off, out=g.t)
        assert np.array_equal(g.t.cpu().numpy(), want) and g.guards_intact()
        assert want[0, 0] == LX.B30 + 1 + off and want[:, 0].max() == n - 1 + off == LX.B31 - 2

        gb = LX.Guarded((4,), torch.int32, dev)
        _lib.check(eng.lib.ovn_best_match(eng._h, _ptr(scores), None, None, n, thr, off, _ptr(gb.t), eng._stream()), "ovn_best_match")
        assert np.array_equal(gb.t.cpu().numpy(), want[0]) and gb.guards_intact()

        # two segments: [0, 8) and [8, n): the second has 2^31 - 16 scores and starts 32 bytes into the buffer (the 16-byte path)
        gs = LX.Guarded((2, k, 4), torch.int32, dev)
        eng.top_k_segments(scores, [0, 8, n], k=k, threshold=thr, out=gs.t)
        seg0 = np.concatenate([records([plant[0]], 0, 0), records([(i, 0.0) for i in range(1, 8)], 0, 0)])
        seg1 = np.concatenate([records([pv for pv in order if pv[0] >= 8], 0, 8), records([(8, 0.0), (9, 0.0), (10, 0.0)], 0, 8)])
        got = gs.t.cpu().numpy()
        assert np.array_equal(got[0], seg0) and np.array_equal(got[1], seg1) and gs.guards_intact()
        # [1, n): 4 bytes into the buffer, so the element-by-element loop walks all 2^31 - 9 scores from position 0 (k = 5: the
        # winners alone, two passes)
        gu = LX.Guarded((2, 5, 4), torch.int32, dev)
        eng.top_k_segments(scores, [0, 1, n], k=5, threshold=thr, out=gu.t)
        un0 = np.concatenate([records([plant[0]], 0, 0), np.array([[-1, 0, 0, 0]] * 4, np.int32)])
        un1 = records([pv for pv in order if pv[0] >= 1], 0, 1)
        got = gu.t.cpu().numpy()
        assert np.array_equal(got[0], un0) and np.array_equal(got[1], un1) and gu.guards_intact()
        del scores, g, gb, gs
    LX.release()


# ---- ovn_mcl_predict ----------------------------------------------------------------------------------------------------------------

def test_mcl_lookup_in_a_grid_of_2_31_cells(eng):
    """cell_frame of 46 340 x 46 340 cells (2 147 395 600, the largest square under the header's cap; 8.6 GB): particles in the first
    rows, in the rows around flat cell 2^30 (byte offset 2^32) and in the last rows, against tests/_mcl_ref.py given those rows."""
    c = LX.BY_NAME["mcl_cells"]
    nx = ny = c.n
    M, P = 50, 64
    LX.need_or_skip(int(9e9))
    dev = eng.device
    mid = LX.straddler(nx, LX.B30)
    groups = [(0, 2), (mid, 2), (ny - 2, 2)]                         # (first row, rows) of the three blocks the particles land in
    rows = [0, 1, mid, mid + 1, ny - 2, ny - 1]
    cols = [0, 1, 17, nx // 2, nx - 2, nx - 1]
    rs = np.random.default_rng(5)
    with _Meter("mcl_predict lookup (%d x %d cells)" % (nx, ny), eng):
        cells = torch.empty(nx * ny, dtype=torch.int32, device=dev)
        for a in range(0, cells.numel(), LX.CHUNK):
            cells[a:a + LX.CHUNK].fill_(-1)
        part = np.zeros((P, 4), np.float32)
        for i in range(P):
            iy, ix = rows[i % 6], cols[(i // 6) % 6]
            part[i] = (ix + 0.5, iy + 0.5, rs.uniform(-3, 3), 1.0)
            if i < 36:     # (36 distinct cells; the later particles share them) a frame, now and then an empty cell, one entry >= M
                cells[iy * nx + ix] = M + 3 if i == 11 else (-1 if i % 7 == 3 else int((iy * 31 + ix * 7) % M))
        part[P - 1, :2] = (-5.0, ny + 9.0)                           # off the map
        parts = torch.from_numpy(part).to(dev)
        outs = [LX.Guarded((P,), torch.int32, dev), LX.Guarded((M,), torch.int32, dev), LX.Guarded((M,), torch.int32, dev),
                LX.Guarded((4,), torch.int32, dev)]
        eng.mcl_predict(parts, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 9, 1, cells, (0.0, 0.0), 1.0, nx, ny, M,
                        particle_frame=outs[0].t, frame_slot=outs[1].t, frame_list=outs[2].t, record=outs[3].t)
        got = parts.cpu().numpy()
        assert np.array_equal(got[:, :2], part[:, :2])               # no motion, no noise: the positions are the planted ones
        want_pf = np.full(P, -1, np.int32)
        iy_all = np.floor(got[:, 1]).astype(np.int64)
        for r0, nr in groups:
            sel = (iy_all >= r0) & (iy_all < r0 + nr) & (got[:, 0] >= 0)
            block = cells[r0 * nx:(r0 + nr) * nx].cpu().numpy()
            want_pf[sel] = MR.lookup(got[sel, 0], got[sel, 1], block, 0.0, 0.0, 1.0, nx, ny, M, cell_offset=r0 * nx)
        lst, slot, rec = MR.distinct(want_pf, M)
        assert (want_pf >= 0).sum() > 40 and len(lst) > 10
        assert np.array_equal(outs[0].t.cpu().numpy(), want_pf) and np.array_equal(outs[1].t.cpu().numpy(), slot)
        assert np.array_equal(outs[2].t.cpu().numpy()[:len(lst)], lst) and np.array_equal(outs[3].t.cpu().numpy(), rec)
        assert all(o.guards_intact() for o in outs)
        del cells, outs
    LX.release()


# ---- the indexed and segmented head routes, and the two head backward calls, over a big pool -----------------------------------------

def test_head_routes_index_a_pool_past_2_31(fixture_npz):
    """A pool of 46 610 feature volumes (8.6 GB), zero except the first and the last four, addressed through lidx / ridx / cand_idx /
    query_idx: the same bits as the same calls on a compact pool of 32 volumes.  A pair's bits depend on its left volume's slot
    modulo 32 (include/ovn_hip.h, ovn_heads), so the compact pool keeps every volume at its slot modulo 32."""
    from overlapnet_amd.engine import OvnEngine
    c = LX.BY_NAME["heads_pool"]
    n, vol = c.n, c.per_item
    assert (n - 4) * vol >= LX.B31 and n % 32 >= 8                    # the last four start past 2^31 and do not collide with slots 0..3
    LX.need_or_skip(int(14e9))
    e = OvnEngine(H, W, 4, device=0)
    try:
        e.load_weights(S.make_test_weights(4, seed=0), S.REFERENCE_MODEL_CFG)
        dev = e.device
        with _Meter("head routes over a pool of %d volumes" % n, e):
            feats = e.leg(torch.from_numpy(S.candidate_images(8, 4, fixture=fixture_npz)).to(dev))
            slots = [0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1]
            big = torch.zeros((n, 360, 128), dtype=torch.float32, device=dev)
            small = torch.zeros((32, 360, 128), dtype=torch.float32, device=dev)
            big[torch.tensor(slots, device=dev)] = feats
            small[torch.tensor([s_ % 32 for s_ in slots], device=dev)] = feats
            lidx = [n - 4, n - 3, n - 2, n - 1, 0, 1, n - 1, 2]
            ridx = [0, n - 1, n - 2, 1, n - 3, n - 4, n - 1, 3]
            cand = [n - 1, 0, n - 2, 3, n - 3, 1, n - 4]               # two segments: 4 candidates for query n - 1, 3 for query 0
            offs, query = [0, 4, 7], [n - 1, 0]
            tgt = [0.9, 0.1, 0.5, 0.8, 0.3, 0.75, 1.0, 0.0]
            bins = [0, 359, 180, 17, 400, -1, 90, 5]

            def run(pool, m):
                ix = lambda a: [v % m if m else v for v in a]
                out = {}
                for prec in ("f16x3", "f32"):
                    e.set_head_precision(prec)
                    r = e.heads(pool, pool, lidx=ix(lidx), ridx=ix(ridx), want_logit=True, want_corr=True)
                    out.update({"heads %s %s" % (prec, k): v for k, v in r.items()})
                    ov, lg = (torch.empty(8, dtype=torch.float32, device=dev) for _ in range(2))
                    li, ri = (torch.tensor(ix(a), dtype=torch.int32, device=dev) for a in (lidx, ridx))
                    _lib.check(e.lib.ovn_delta_head(e._h, _ptr(pool), _ptr(li), _ptr(pool), _ptr(ri), 8, _ptr(ov), _ptr(lg), e._stream()),
                               "ovn_delta_head")
                    out.update({"delta %s overlap" % prec: ov, "delta %s logit" % prec: lg})
                    r = e.heads_segments(pool, pool, ix(cand), ix(query), offs, want_logit=True, want_corr=True)
                    out.update({"segments %s %s" % (prec, k): v for k, v in r.items()})
                e.set_head_precision("f16x3")
                r = e.corr_head(pool, pool, lidx=ix(lidx), ridx=ix(ridx), want_corr=True)
                out.update({"corr " + k: v for k, v in r.items()})
                r = e.delta_head_grad(pool, pool, tgt, lidx=ix(lidx), ridx=ix(ridx))
                out.update({"head grad " + k: r[k] for k in ("flat", "loss", "overlap")})
                r = e.heads_feature_grad(pool, pool, tgt, yaw_bins=bins, lidx=ix(lidx), ridx=ix(ridx), want_head_grads=True)
                out.update({"feature grad " + k: r[k] for k in ("dfeat_l", "dfeat_r", "loss", "overlap", "corr", "flat")})
                return out

            got, want = run(big, 0), run(small, 32)
            # the same heads call once more with every output between guard bands
            go, gy, gl, gc = (LX.Guarded(sh, dt, dev) for sh, dt in (((8,), torch.float32), ((8,), torch.int32), ((8,), torch.float32),
                                                                     ((8, 360), torch.float32)))
            li, ri = (torch.tensor(a, dtype=torch.int32, device=dev) for a in (lidx, ridx))
            _lib.check(e.lib.ovn_heads(e._h, _ptr(big), _ptr(li), _ptr(big), _ptr(ri), 8, _ptr(go.t), _ptr(gy.t), _ptr(gl.t), _ptr(gc.t),
                                       e._stream()), "ovn_heads")
            for gg, key in ((go, "overlap"), (gy, "yaw"), (gl, "logit"), (gc, "corr")):
                assert gg.guards_intact() and torch.equal(gg.bits, want["heads f16x3 " + key].contiguous().view(torch.int32).reshape(-1)), key
            assert set(got) == set(want) and len(got) > 25
            for k in sorted(got):
                a, b = got[k].contiguous().view(torch.int32), want[k].contiguous().view(torch.int32)
                assert a.shape == b.shape and torch.equal(a, b), k
                assert bool(torch.isfinite(got[k].float()).all()), k
            ov = got["heads f16x3 overlap"].cpu().numpy()
            assert ov.min() > 0.0 and ov.max() < 1.0 and len(np.unique(ov)) >= 4         # real pairs, not eight copies of one value
            assert float(got["feature grad dfeat_l"].abs().max()) > 0.0
            del big, small, got, want
    finally:
        e.close()
        LX.release()


# ---- ovn_render_scans ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["exhaustive", "hierarchy"])
def test_render_scans_past_2_31(eng, route):
    """9 325 poses at 64 x 900, all non-finite (the header: an all-empty scan) except the boundary ones, on the scene of
    tests/_render_ref.py: vertex and stacked (q * 4) pass 2^31, normal (q * 3) and the others pass byte offset 2^32.  The small call
    is what tests/test_gpu_render.py ties to the float32 statement; the statement itself takes seconds per 64 x 900 pose, so (d) is
    left to that module."""
    import _render_ref as R
    from overlapnet_amd.mesh import TriangleMesh
    c, reals = _reals("render_vertex")
    n = c.n
    LX.need_or_skip(int(30e9))
    dev = eng.device
    exhaustive = route == "exhaustive"
    mesh = TriangleMesh(*R.scene(0))
    poses = np.full((n, 4, 4), np.nan, np.float64)
    poses[1::2] = np.inf                                              # both kinds of non-finite entries
    poses[reals] = R.scene_poses(len(reals), seed=3)
    with _Meter("render_scans %s (n = %d)" % (route, n), eng):
        small = eng.render_scans(mesh, poses[reals], H, W, fov_up=R.FOV_UP, fov_down=R.FOV_DOWN, max_range=R.MAX_RANGE,
                                 want=("range", "tri_id", "vertex", "normal"), stacked_flags=(True, True), exhaustive=exhaustive)
        assert 0.5 < float((small["tri_id"] >= 0).float().mean()) < 0.999
        md = mesh.device(eng, with_bvh=not exhaustive)
        nodes, order, leaves = (None, None, 0) if exhaustive else (md["nodes"], md["order"], md["leaves"])
        tabs = eng._direction_tables(H, W, R.FOV_UP, R.FOV_DOWN)
        p = torch.from_numpy(poses).to(dev)
        g = {"range": LX.Guarded((n, H, W), torch.float32, dev), "tri_id": LX.Guarded((n, H, W), torch.int32, dev),
             "vertex": LX.Guarded((n, H, W, 4), torch.float32, dev), "normal": LX.Guarded((n, H, W, 3), torch.float32, dev),
             "stacked": LX.Guarded((n, H, W, 4), torch.float32, dev)}
        _lib.check(eng.lib.ovn_render_scans(eng._h, _ptr(md["vertices"]), mesh.n_vertices, _ptr(md["triangles"]), mesh.n_triangles,
                                            _ptr(nodes), _ptr(order), int(leaves), _ptr(p), n, H, W, _ptr(tabs[0]), _ptr(tabs[1]),
                                            _ptr(tabs[2]), _ptr(tabs[3]), float(R.MAX_RANGE), _ptr(g["range"].t), _ptr(g["tri_id"].t),
                                            _ptr(g["vertex"].t), _ptr(g["normal"].t), _ptr(g["stacked"].t), 1, 1, 0, 0, eng._stream()),
                   "ovn_render_scans")
        for k, ch in (("range", 1), ("tri_id", 1), ("vertex", 4), ("normal", 3), ("stacked", 4)):
            _assert_clean(k, LX.check_items(g[k], HW * ch, n, reals, _bits(small[k]), -1 if k == "tri_id" else M1))
        del g, p, small
    LX.release()


# ---- ovn_leg_forward_train, ovn_leg_backward ----------------------------------------------------------------------------------------

def test_leg_train_layer_major_activations_past_2_31(fixture_npz):
    """2 260 scans of the reference leg (951 776 activations each): 2.15e9 activations, layer-major (block li at n * act_off[li]).  Real scans are the first and
    the last scan block, every other scan is an all -1 image with a zero dfeat.  Forward: every layer block == the small call's
    (real scans) resp. the empty image's activations.  Backward: the empty scans add exact zeros (dfeat = 0 through every ReLU mask
    and product) and the real scans fill the same two scan blocks as in the small call, so the gradients must EQUAL the small
    call's (float equality: a sum that is -0 alone may come back +0 next to added zeros)."""
    from overlapnet_amd.engine import OvnEngine
    n, sb = LX.LEG_TRAIN_N, LX.LEG_TRAIN_BLOCK
    LX.need_or_skip(int(13e9))
    e = OvnEngine(H, W, 4, device=0)
    try:
        e.load_weights(S.make_test_weights(4, seed=0), S.REFERENCE_MODEL_CFG)
        dev = e.device
        shapes = e.leg_activation_shapes()
        sizes = [a * b * c for a, b, c in shapes]
        assert sizes == LX.leg_activation_sizes(H, W, 4, S.REFERENCE_MODEL_CFG) and n * sum(sizes) >= LX.B31
        reals = list(range(sb)) + list(range(n - sb, n))
        with _Meter("leg_forward_train + leg_backward (n = %d)" % n, e):
            real = torch.from_numpy(S.candidate_images(2 * sb, 4, fixture=fixture_npz)).to(dev)
            small_in = torch.cat([real, torch.full((1, H, W, 4), -1.0, device=dev)])
            imgs = torch.full((n, H, W, 4), -1.0, dtype=torch.float32, device=dev)
            imgs[torch.tensor(reals, device=dev)] = real
            g = LX.Guarded((n * sum(sizes),), torch.float32, dev)
            _lib.check(e.lib.ovn_leg_forward_train(e._h, _ptr(imgs), n, _ptr(g.t), e._stream()), "ovn_leg_forward_train")
            small = e.leg_forward_train(small_in)                       # 2 sb real scans, then the empty image
            acts, off = [], 0
            res = {"guards": g.guards_intact(), "sentinel_left": g.count_sentinel(), "real_diff": 0, "empty_diff": 0}
            for (a, b, c), sz, sm in zip(shapes, sizes, small):
                smb = _bits(sm)
                r = LX.check_rows(g.bits[off:off + n * sz].view(n, sz), reals, smb[:-1], smb[-1])
                res["real_diff"] += r["real_diff"]
                res["empty_diff"] += r["empty_diff"]
                acts.append(g.t[off:off + n * sz].view(n, a, b, c))
                off += n * sz
            _assert_clean("activations", res)
            assert off * 4 >= 2 * LX.B32 and float(acts[-1][n - 1].abs().max()) > 0.0

            rs = np.random.default_rng(11)
            d_real = torch.from_numpy(rs.standard_normal((2 * sb, 360, 128)).astype(np.float32)).to(dev)
            dfeat = torch.zeros((n, 360, 128), dtype=torch.float32, device=dev)
            dfeat[torch.tensor(reals, device=dev)] = d_real
            import ctypes
            g_flat = LX.Guarded((sum(int(np.prod(sh)) for sh in e.leg_param_shapes()),), torch.float32, dev)
            _lib.check(e.lib.ovn_leg_backward(e._h, _ptr(imgs), ctypes.c_void_p(acts[0].data_ptr()), n, _ptr(dfeat), _ptr(g_flat.t), 0,
                                              e._stream()), "ovn_leg_backward")
            got = g_flat.t
            assert g_flat.guards_intact() and g_flat.count_sentinel() == 0
            want = e.leg_backward(small_in[:-1].contiguous(), e.leg_forward_train(small_in[:-1].contiguous()), d_real)["flat"]
            differ = int((got != want).sum().item())
            print("[large extent]   leg_backward: %d of %d gradient elements differ from the small call, largest |g| %.3g"
                  % (differ, got.numel(), float(want.abs().max())))
            assert bool(torch.isfinite(got).all()) and float(want.abs().max()) > 0.0 and differ == 0
            assert g.guards_intact()
            del g, acts, imgs, dfeat, small
    finally:
        e.close()
        LX.release()


# ---- ovn_project: the offsets into `points` and the per-point scratch ----------------------------------------------------------------

def test_project_points_offset_past_2_31(eng, fixture_npz):
    """Two scans, the first a dummy of 537 000 000 points at (0, 0, 0), which the range filter drops, the second real, with `idx`
    requested: offsets[scan] * 4 and (beg + p) * 4 pass 2^31 elements of `points`, scan * max_points + p walks 4.3 GB of kept-point
    numbering, scan * blocks_per_scan + b two million block counts per scan."""
    d = LX.PROJECT_DUMMY_POINTS
    cloud = S.z_rotated(fixture_npz["points_1"], 111)
    LX.need_or_skip(int(14e9))
    dev = eng.device
    with _Meter("project, %d dummy points in front of the real scan" % d, eng):
        pts = torch.zeros((d + len(cloud), 4), dtype=torch.float32, device=dev)
        pts[d:] = torch.from_numpy(cloud).to(dev)
        offs = torch.tensor([0, d, d + len(cloud)], dtype=torch.int64, device=dev)
        shapes = {"range": ((2, H, W), torch.float32), "vertex": ((2, H, W, 4), torch.float32), "intensity": ((2, H, W), torch.float32),
                  "idx": ((2, H, W), torch.int32), "normal": ((2, H, W, 3), torch.float32), "stacked": ((2, H, W, 5), torch.float32)}
        g = {k: LX.Guarded(sh, dt, dev) for k, (sh, dt) in shapes.items()}
        _project(eng, pts, offs, 2, d, rng=g["range"].t, vtx=g["vertex"].t, itn=g["intensity"].t, idx=g["idx"].t, nrm=g["normal"].t,
                 stk=g["stacked"].t, flags=(1, 1, 1))
        small = _small(eng, [cloud], ("range", "vertex", "intensity", "idx", "normal"), (1, 1, 1))
        for k, (sh, _) in shapes.items():
            per = int(np.prod(sh[1:]))
            _assert_clean(k, LX.check_items(g[k], per, 2, [1], _bits(small[k]), -1 if k == "idx" else M1))
        o_rng, o_vtx, o_itn, _ = O.range_projection(cloud)
        assert np.array_equal(g["range"].t[1].cpu().numpy(), o_rng) and np.array_equal(g["vertex"].t[1].cpu().numpy(), o_vtx)
        assert np.array_equal(g["intensity"].t[1].cpu().numpy(), o_itn) and int((g["idx"].t[1] >= 0).sum()) > 20000
        del pts, g, small
    LX.release()


def test_project_semantic_output_past_2_31(eng, fixture_npz):
    """q * n_classes and q * C: the (n, H, W, 20) probability image and the (n, H, W, 25) stacked input (depth | normals |
    probabilities | intensity) of 1 870 scans, through the 16-byte row kernel (n_classes = 20)."""
    c, reals = _reals("semantic_out", extra=LX.real_items(LX.BY_NAME["semantic_stacked"]))
    n, nc = c.n, 20
    assert n == LX.BY_NAME["semantic_stacked"].n
    LX.need_or_skip(int(23e9))
    clouds = _clouds(fixture_npz, reals)
    dev = eng.device
    with _Meter("project_semantic semantic (n = %d)" % n, eng):
        pts, offs, mx = _batch(clouds, reals, n, dev)
        sp, so, smx = _batch(clouds, list(range(len(clouds))), len(clouds), dev)
        assert torch.equal(pts, sp)                                    # empty scans add no points: the same points and rows
        probs = torch.from_numpy(np.random.default_rng(2).random((pts.shape[0], nc), np.float32)).to(dev)
        g_sem, g_sid = LX.Guarded((n, H, W, nc), torch.float32, dev), LX.Guarded((n, H, W), torch.int32, dev)
        g_stk = LX.Guarded((n, H, W, 5 + nc), torch.float32, dev)
        _lib.check(eng.lib.ovn_project_semantic(eng._h, _ptr(pts), _ptr(offs), n, mx, H, W, *GEO, _ptr(probs), nc, None, None, None,
                                                None, None, _ptr(g_sem.t), _ptr(g_sid.t), _ptr(g_stk.t), 1, 1, 1, 1, eng._stream()),
                   "ovn_project_semantic")
        small = eng.project(sp, so, smx, H, W, *GEO, want=("semantic", "sem_idx"), stacked_flags=(True, True, True, True),
                            probs=probs, n_classes=nc)
        _assert_clean("stacked", LX.check_items(g_stk, HW * (5 + nc), n, reals, _bits(small["stacked"]), M1))
        assert torch.equal(g_stk.t[n - 1][..., 4:4 + nc], g_sem.t[n - 1])
        del g_stk
        _assert_clean("semantic", LX.check_items(g_sem, HW * nc, n, reals, _bits(small["semantic"]), M1))
        _assert_clean("sem_idx", LX.check_items(g_sid, HW, n, reals, _bits(small["sem_idx"]), -1))
        # (d) the last item: probs[sem_idx] where a point landed, as the reference gathers it (gen_semantic_data.py:44)
        sid = g_sid.t[n - 1].cpu().numpy()
        rows = probs[int(offs[n - 1]):].cpu().numpy()
        want = np.where((sid >= 0)[..., None], rows[np.maximum(sid, 0)], np.float32(-1))
        assert np.array_equal(g_sem.t[n - 1].cpu().numpy(), want) and (sid >= 0).mean() > 0.5
        del g_sem, g_sid, pts, probs, small
    LX.release()


# ---- ovn_tsdf_triangles (count mode), ovn_tsdf_bricks on the largest volume ----------------------------------------------------------

def test_tsdf_count_and_bricks_on_the_largest_volume(eng):
    """1290^3 = 2 146 689 000 samples, the largest cube under the header's cap (2 x 8.6 GB): fresh (tsdf 1, weight 0) except three
    blocks of 12^3 samples with weight 1 and a seeded tsdf pattern -- at the first corner, around sample 2^30 (byte offset 2^32) and at
    the last corner.  The triangle count is three times that of a 16^3 volume holding the block alone (only cells inside a block are
    live); the brick mask is known in closed form."""
    c = LX.BY_NAME["tsdf_volume"]
    N, B = c.n, 12
    mid = LX.straddler(c.per_item, LX.B30)                            # the slab that holds sample 2^30
    bases = [(0, 0, 0), (mid - 5, 641, 322), (N - B, N - B, N - B)]   # (k, j, i) of each block's first sample
    assert bases[1][0] <= mid < bases[1][0] + B and (((N - B) * N + (N - B)) * N + N - B) * 4 >= LX.B32
    LX.need_or_skip(int(18e9))
    dev = eng.device
    rs = np.random.default_rng(4)
    block = torch.from_numpy(rs.uniform(-1, 1, (B, B, B)).astype(np.float32)).to(dev)
    with _Meter("tsdf_triangles count + tsdf_bricks (%d^3 samples)" % N, eng):
        tsdf = torch.empty((N, N, N), dtype=torch.float32, device=dev)
        weight = torch.empty((N, N, N), dtype=torch.float32, device=dev)
        rows = max(1, LX.CHUNK // (N * N))
        for a in range(0, N, rows):
            tsdf[a:a + rows].fill_(1.0)
            weight[a:a + rows].zero_()
        for k, j, i in bases:
            tsdf[k:k + B, j:j + B, i:i + B] = block
            weight[k:k + B, j:j + B, i:i + B] = 1.0
        st = torch.ones((16, 16, 16), dtype=torch.float32, device=dev)
        sw = torch.zeros((16, 16, 16), dtype=torch.float32, device=dev)
        st[2:2 + B, 2:2 + B, 2:2 + B] = block
        sw[2:2 + B, 2:2 + B, 2:2 + B] = 1.0
        _, t_small = eng.tsdf_triangles(st, sw, (0.0, 0.0, 0.0), 0.1, min_weight=1.0, capacity=0)
        g_cnt, cnt = _guarded64((1,), torch.int64, dev)
        vx, vy, vz, org = eng._tsdf_volume_args("tsdf_triangles", tsdf, weight, (0.0, 0.0, 0.0))
        _lib.check(eng.lib.ovn_tsdf_triangles(eng._h, _ptr(tsdf), _ptr(weight), vx, vy, vz, org, 0.1, 1.0, None, 0, _ptr(cnt),
                                              eng._stream()), "ovn_tsdf_triangles")
        t_big = int(cnt.item())
        assert g_cnt.guards_intact()
        print("[large extent]   triangles: %d in the volume, %d per block" % (t_big, t_small))
        assert t_small > 1000 and t_big == 3 * t_small

        nb = -(-N // 8)
        assert nb ** 3 % 4 == 0
        g = LX.Guarded((nb ** 3 // 4,), torch.int32, dev)
        mask = g.bits.view(torch.uint8).view(nb, nb, nb)
        eng.tsdf_bricks(weight, 1.0, out=mask)
        want = np.zeros((nb, nb, nb), np.uint8)
        for k, j, i in bases:
            want[k // 8:(k + B - 1) // 8 + 1, j // 8:(j + B - 1) // 8 + 1, i // 8:(i + B - 1) // 8 + 1] = 1
        assert int(want.sum()) == 8 + 8 + 27 and torch.equal(mask, torch.from_numpy(want).to(dev)) and g.guards_intact()
        del tsdf, weight, g, mask
    LX.release()


# ---- ovn_gt_pair_counts -------------------------------------------------------------------------------------------------------------

def test_gt_pair_counts_past_2_30_pairs(eng, fixture_npz):
    """32 769 x 32 769 pairs (just above 2^30: the counts pass byte offset 2^32; the header caps the pairs at 2^31 - 1), every scan
    empty except the last two.  A pair with an empty reference scan counts nothing, a real reference against an empty frame (range
    image all -1) counts nothing either: everything is 0 except the 2 x 2 corner, which must equal the call on the two scans alone."""
    c = LX.BY_NAME["gt_pair_counts"]
    n = c.n
    assert n * n > LX.B30
    LX.need_or_skip(int(14e9))
    dev = eng.device
    clouds = [S.z_rotated(fixture_npz["points_0"], 3), fixture_npz["points_1"]]
    with _Meter("gt_pair_counts (%d x %d pairs)" % (n, n), eng):
        sp, so, smx = _batch(clouds, [0, 1], 2, dev)
        eye2 = torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1).contiguous()
        own = eng.gt_range_images(sp, so, smx)
        small = eng.gt_pair_counts(sp, so, eye2, eye2, own)                       # (2, 2)
        assert int(small.min()) > 1000 and int(small[0, 0]) != int(small[1, 1])
        pts, offs, _ = _batch(clouds, [n - 2, n - 1], n, dev)
        eye = torch.eye(4, dtype=torch.float64, device=dev).repeat(n, 1, 1).contiguous()
        cur = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        rows = max(1, LX.CHUNK // HW)
        for a in range(0, n, rows):
            cur[a:a + rows].fill_(-1.0)
        cur[n - 2:] = own
        g = LX.Guarded((n, n), torch.int32, dev)
        _lib.check(eng.lib.ovn_gt_pair_counts(eng._h, _ptr(pts), _ptr(offs), n, _ptr(eye), _ptr(eye), _ptr(cur), None, n, None, n, H, W,
                                              *GEO, _ptr(g.t), eng._stream()), "ovn_gt_pair_counts")
        want = torch.zeros((2, n), dtype=torch.int32, device=dev)
        want[:, n - 2:] = small
        _assert_clean("pair counts", LX.check_items(g, n, n, [n - 2, n - 1], want, 0))
        del g, cur, eye, pts
    LX.release()


# ---- ovn_project_semantic: the probability rows -------------------------------------------------------------------------------------

def test_project_semantic_probability_rows_past_2_31(eng, fixture_npz):
    """Two scans, the first a dummy of 107 400 000 points at the origin (no depth: kept by neither filter), the second real:
    (offsets[scan] + sem_idx) * 20 passes 2^31 elements of the 8.6 GB of probability rows.  All outputs, the stacked one included."""
    d, nc = LX.SEMANTIC_DUMMY_POINTS, 20
    cloud = S.z_rotated(fixture_npz["points_0"], 77)
    LX.need_or_skip(int(12e9))
    dev = eng.device
    with _Meter("project_semantic, %d dummy points in front of the real scan" % d, eng):
        pts = torch.zeros((d + len(cloud), 4), dtype=torch.float32, device=dev)
        pts[d:] = torch.from_numpy(cloud).to(dev)
        rows = torch.from_numpy(np.random.default_rng(6).random((len(cloud), nc), np.float32)).to(dev)
        probs = torch.zeros((d + len(cloud), nc), dtype=torch.float32, device=dev)
        probs[d:] = rows
        offs = torch.tensor([0, d, d + len(cloud)], dtype=torch.int64, device=dev)
        shapes = {"range": ((2, H, W), torch.float32), "idx": ((2, H, W), torch.int32), "normal": ((2, H, W, 3), torch.float32),
                  "semantic": ((2, H, W, nc), torch.float32), "sem_idx": ((2, H, W), torch.int32),
                  "stacked": ((2, H, W, 5 + nc), torch.float32)}
        g = {k: LX.Guarded(sh, dt, dev) for k, (sh, dt) in shapes.items()}
        _lib.check(eng.lib.ovn_project_semantic(eng._h, _ptr(pts), _ptr(offs), 2, d, H, W, *GEO, _ptr(probs), nc, _ptr(g["range"].t),
                                                None, None, _ptr(g["idx"].t), _ptr(g["normal"].t), _ptr(g["semantic"].t),
                                                _ptr(g["sem_idx"].t), _ptr(g["stacked"].t), 1, 1, 1, 1, eng._stream()),
                   "ovn_project_semantic")
        sp, so, smx = _batch([cloud], [0], 1, dev)
        small = eng.project(sp, so, smx, H, W, *GEO, want=("range", "idx", "normal", "semantic", "sem_idx"),
                            stacked_flags=(True, True, True, True), probs=rows, n_classes=nc)
        for k, (sh, dt) in shapes.items():
            _assert_clean(k, LX.check_items(g[k], int(np.prod(sh[1:])), 2, [1], _bits(small[k]), -1 if dt == torch.int32 else M1))
        sid = g["sem_idx"].t[1].cpu().numpy()
        want = np.where((sid >= 0)[..., None], rows.cpu().numpy()[np.maximum(sid, 0)], np.float32(-1))
        assert np.array_equal(g["semantic"].t[1].cpu().numpy(), want) and (sid >= 0).mean() > 0.5
        del pts, probs, g, small
    LX.release()


# ---- ovn_tsdf_raycast at many poses -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["volume", "bricks"])
def test_tsdf_raycast_poses_past_2_31(eng, route):
    """9 325 poses at 64 x 900 on the sphere volume of tests/_raycast_ref.py, all non-finite except the boundary ones, without and
    with the brick mask: the outputs of the render case.  The small call is what tests/test_gpu_raycast.py ties to the statement."""
    import _raycast_ref as RC
    c, reals = _reals("raycast_vertex")
    n = c.n
    LX.need_or_skip(int(28e9))
    dev = eng.device
    v = RC.volume_case("sphere")
    tsdf, weight = (torch.from_numpy(v[k]).to(dev) for k in ("tsdf", "weight"))
    mask = eng.tsdf_bricks(weight, RC.MIN_WEIGHT) if route == "bricks" else None
    poses = np.full((n, 4, 4), np.nan, np.float64)
    poses[1::2] = np.inf
    poses[reals] = v["poses"][[0, 1, 0, 1, 0, 1][:len(reals)]]
    for j, i in enumerate(reals):                                       # no two real poses alike
        poses[i, :3, 3] += 0.01 * j
    kw = dict(proj_h=H, proj_w=W, min_range=v["min_range"], max_range=v["max_range"], step=v["step"], min_weight=RC.MIN_WEIGHT,
              bricks=mask, want=("range", "vertex", "normal"), stacked_flags=(True, True))
    with _Meter("tsdf_raycast %s (n = %d)" % (route, n), eng):
        small = eng.tsdf_raycast(tsdf, weight, v["origin"], v["voxel"], poses[reals], **kw)
        assert 0.001 < float((small["range"] > 0).float().mean()) < 0.999
        g = {"range": LX.Guarded((n, H, W), torch.float32, dev), "vertex": LX.Guarded((n, H, W, 4), torch.float32, dev),
             "normal": LX.Guarded((n, H, W, 3), torch.float32, dev), "stacked": LX.Guarded((n, H, W, 4), torch.float32, dev)}
        eng.tsdf_raycast(tsdf, weight, v["origin"], v["voxel"], poses, out={k: g[k].t for k in ("range", "vertex", "normal")},
                         stacked_out=g["stacked"].t, **kw)
        for k, ch in (("range", 1), ("vertex", 4), ("normal", 3), ("stacked", 4)):
            _assert_clean(k, LX.check_items(g[k], HW * ch, n, reals, _bits(small[k]), M1))
        del g, small
    LX.release()


# ---- the correlation head's (n, 360) output -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["direct", "spectral"])
def test_corr_head_output_past_2_31(route, fixture_npz):
    """5 965 300 pairs indexed into a pool of 10 volumes: corr (n, 360) passes 2^31 elements.  Every pair is one of 100 (l, r)
    combinations, so EVERY row is compared, on the device, with the small call on those 100 pairs (a pair's result does not depend on
    the batch); the last pair against the oracle's correlation at the tolerance of tests/test_gpu_parity.py (2e-5 of the largest value)."""
    from overlapnet_amd.engine import OvnEngine
    c = LX.BY_NAME["corr_out"]
    n, P = c.n, 10
    LX.need_or_skip(int(10e9))
    e = OvnEngine(H, W, 4, device=0)
    try:
        e.load_weights(S.make_test_weights(4, seed=0), S.REFERENCE_MODEL_CFG)
        dev = e.device
        with _Meter("corr_head %s (n = %d)" % (route, n), e):
            feats = e.leg(torch.from_numpy(S.candidate_images(P, 4, fixture=fixture_npz)).to(dev))
            pool = e.spectrum(feats) if route == "spectral" else feats
            call = e.lib.ovn_corr_head_spectral if route == "spectral" else e.lib.ovn_corr_head
            gen = torch.Generator(device=dev).manual_seed(3)
            li = torch.randint(0, P, (n,), generator=gen, device=dev, dtype=torch.int32)
            ri = torch.randint(0, P, (n,), generator=gen, device=dev, dtype=torch.int32)
            li[-1], ri[-1] = 3, 7
            g_corr, g_yaw = LX.Guarded((n, 360), torch.float32, dev), LX.Guarded((n,), torch.int32, dev)
            _lib.check(call(e._h, _ptr(pool), _ptr(li), _ptr(pool), _ptr(ri), n, _ptr(g_yaw.t), _ptr(g_corr.t), e._stream()), route)
            al = torch.arange(P * P, device=dev, dtype=torch.int32)
            t_corr, t_yaw = LX.Guarded((P * P, 360), torch.float32, dev), LX.Guarded((P * P,), torch.int32, dev)
            tl, tr = (al // P).contiguous(), (al % P).contiguous()       # held: a pointer does not keep a temporary alive
            _lib.check(call(e._h, _ptr(pool), _ptr(tl), _ptr(pool), _ptr(tr), P * P,
                            _ptr(t_yaw.t), _ptr(t_corr.t), e._stream()), route)
            table, ytab = t_corr.bits.view(P * P, 360), t_yaw.bits
            bad = ybad = 0
            rows = LX.CHUNK // 512
            view = g_corr.bits.view(n, 360)
            for a in range(0, n, rows):
                key = (li[a:a + rows].long() * P + ri[a:a + rows].long())
                bad += int((view[a:a + rows] != table[key]).sum().item())
                ybad += int((g_yaw.bits[a:a + rows] != ytab[key]).sum().item())
            print("[large extent]   %d corr words and %d yaw bins differ from the small call" % (bad, ybad))
            assert bad == 0 and ybad == 0 and g_corr.guards_intact() and g_yaw.guards_intact()
            assert t_corr.guards_intact() and g_corr.count_sentinel() == 0 and len(torch.unique(ytab)) > 3
            fv = feats.cpu().numpy().astype(np.float64).reshape(P, 1, 360, 128)
            ref = O.correlation_head_forward(fv[3:4], fv[7:8])[0]
            got = g_corr.t[n - 1].cpu().numpy()
            err = float(np.max(np.abs(got - ref)) / (np.max(np.abs(ref)) + 1e-30))
            print("[large extent]   last pair vs the oracle: relative error %.3g (allowed 2e-5)" % err)
            assert err < 2e-5
            del g_corr, g_yaw, li, ri
    finally:
        e.close()
        LX.release()


# ---- ovn_tsdf_integrate, ovn_tsdf_triangles (write mode), ovn_tsdf_bricks, ovn_tsdf_raycast on a volume past 2^30 samples -----------------

def test_tsdf_far_block_past_2_30_samples(eng):
    """A volume of 1024 x 1024 x 1072 samples (2 x 4.5 GB): slab 1024 starts at sample 2^30, byte offset 2^32.  Two scans of
    tests/_tsdf_ref.py (ranges scaled to a quarter, max_range 3 m) are fused from poses inside the block of 48^3 samples at
    (488, 488, 1024): every sample they can touch lies inside it.  The block against the statement GIVEN THAT BLOCK (index_offset),
    bit for bit off the samples the statement marks ambiguous; every sample outside it still fresh; then the triangles (write
    mode), the brick mask and ray-cast views (without and with the mask) of the fused volume against their statements on the block."""
    import _raycast_ref as RC
    import _tsdf_ref as T
    c = LX.BY_NAME["tsdf_far_block"]
    nx = ny = 1024
    nz = c.n
    (i0, j0, k0), E = LX.TSDF_BLOCK, LX.TSDF_BLOCK_EDGE
    off = (i0, j0, k0)
    origin = np.array([-100.0, -99.0, -215.0])
    vox, trunc, mr = T.VOXEL, T.TRUNC, 3.0
    LX.need_or_skip(int(19e9))
    dev = eng.device
    rng, poses = T.scans(16, 90, 2)
    rng = (rng * np.float32(0.25)).astype(np.float32)
    centre = origin + (np.array(off) + E / 2) * vox
    poses = poses.copy()
    poses[:, :3, 3] = [centre + [0.13, -0.21, 0.08], centre + [-0.3, 0.17, -0.11]]
    blk = (slice(k0, k0 + E), slice(j0, j0 + E), slice(i0, i0 + E))
    one = LX.f32_bits(1.0)
    with _Meter("tsdf far block (%d x %d x %d samples)" % (nx, ny, nz), eng):
        g_t, g_w = LX.Guarded((nz, ny, nx), torch.float32, dev), LX.Guarded((nz, ny, nx), torch.float32, dev)
        rows = max(1, LX.CHUNK // (nx * ny))
        for a in range(0, nz, rows):
            g_t.t[a:a + rows].fill_(1.0)
            g_w.t[a:a + rows].zero_()
        eng.tsdf_integrate(g_t.t, g_w.t, origin, vox, trunc, T.MAX_WEIGHT, torch.from_numpy(rng).to(dev), poses, max_range=mr)
        bt, bw = g_t.t[blk].contiguous(), g_w.t[blk].contiguous()
        touched = int((bw > 0).sum().item())
        assert g_t.guards_intact() and g_w.guards_intact()
        # (c) outside the block everything is fresh: the words that changed in the whole volume are the block's
        assert g_t.count_not(one) == int((bt.view(torch.int32) != one).sum().item())
        assert g_w.count_not(0) == touched and touched > 2000
        ref = T.integrate(*T.fresh((E, E, E)), origin, vox, trunc, T.MAX_WEIGHT, rng, poses, max_range=mr, ambiguous=True,
                          index_offset=off)
        ok = ~ref["ambiguous"]
        ht, hw = bt.cpu().numpy(), bw.cpu().numpy()
        print("[large extent]   integrate: %d samples touched, %d ambiguous" % (touched, int((~ok).sum())))
        assert np.array_equal(ht.view(np.int32)[ok], ref["tsdf"].view(np.int32)[ok]) and np.array_equal(hw[ok], ref["weight"][ok])
        assert (~ok).mean() < 0.05

        # triangles, write mode, into a guarded buffer
        _, total = eng.tsdf_triangles(g_t.t, g_w.t, origin, vox, min_weight=1.0, capacity=0)
        want = T.triangles(ht, hw, origin, vox, 1.0, index_offset=off)
        assert total == len(want) > 500
        g_tri = LX.Guarded((total, 3, 3), torch.float32, dev)
        tri, t2 = eng.tsdf_triangles(g_t.t, g_w.t, origin, vox, min_weight=1.0, out=g_tri.t)
        assert t2 == total and np.array_equal(tri.cpu().numpy().view(np.int32), want.view(np.int32)) and g_tri.guards_intact()

        # bricks
        nb = (nz // 8, ny // 8, nx // 8)
        g_m = LX.Guarded((nb[0] * nb[1] * nb[2] // 4,), torch.int32, dev)
        mask = g_m.bits.view(torch.uint8).view(*nb)
        eng.tsdf_bricks(g_w.t, RC.MIN_WEIGHT, out=mask)
        bmask = RC.bricks(hw, RC.MIN_WEIGHT)
        sub = mask[k0 // 8:(k0 + E) // 8, j0 // 8:(j0 + E) // 8, i0 // 8:(i0 + E) // 8]
        assert np.array_equal(sub.cpu().numpy(), bmask) and int(mask.sum().item()) == int(bmask.sum()) > 0 and g_m.guards_intact()

        # ray casting: from inside the block, from outside the volume, and a non-finite pose
        view = RC.three_poses(ht, hw, origin + np.array(off) * vox, vox)
        kw = dict(min_range=0.3 * vox, max_range=2.0 * E * vox, step=vox, min_weight=RC.MIN_WEIGHT)
        refc = RC.raycast(ht, hw, origin, vox, view, 16, 90, index_offset=off, full_shape=(nx, ny, nz), **kw)
        assert (refc["range"][:2] > 0).sum() > 50 and (refc["range"][2] < 0).all()
        for m in (None, mask):
            g_r, g_v = LX.Guarded((3, 16, 90), torch.float32, dev), LX.Guarded((3, 16, 90, 4), torch.float32, dev)
            eng.tsdf_raycast(g_t.t, g_w.t, origin, vox, view, proj_h=16, proj_w=90, fov_up=RC.R.FOV_UP, fov_down=RC.R.FOV_DOWN, bricks=m,
                             want=(), out={"range": g_r.t, "vertex": g_v.t}, **kw)
            assert np.array_equal(g_r.t.cpu().numpy().view(np.int32), refc["range"].view(np.int32))
            assert np.array_equal(g_v.t.cpu().numpy().view(np.int32), refc["vertex"].view(np.int32))
            assert g_r.guards_intact() and g_v.guards_intact()
        del g_t, g_w, g_tri, g_m, mask, sub
    LX.release()
